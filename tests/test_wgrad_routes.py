"""Which kernel every weight gradient runs (csrc/wgrad.hip wgrad_route), read back as text through the emulator-only export
``emu_wgrad_route`` — no launch, microseconds — and compared with what the C entries then launch (the emulator's launch trace).

* Every branch of the route at the least shape that reaches it: the route the query predicts is the first-stage kernel of the trace,
  instantiation and grid, and the second stage is the route's; at 256 and at 8 CUs.
* The thresholds (tile kernels from 2048 / 32768 positions, the tap split below 50000, 4 x 6 GEMM tiles, operand alignment) at their edges.
* The workspace queries, which see neither grid nor stride, cover the scratch of every route their arguments can reach.
* The convolution layers of the bench's training step (dtu_pretrain at 512x640, three views) take the kernels that the kernel table of
  the commit BEFORE the route function shows (profiles/wgrad_route_refactor_kernels_parent.csv: the library's rows of a
  ``rocprofv3 --kernel-trace --stats`` of ``bench.py --train``); the test recounts the table, so the pinned expectation cannot drift."""
import collections
import csv
import ctypes as C
import itertools
import os
import re

import pytest
import torch

from emu_lib import emu_cu_count, emu_lib, emu_trace

PROFILES = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles")
Route = collections.namedtuple("Route", "name scratch_bytes atomic second_stage blocks cols chunks tiles_a tiles_b tiles_y tiles_x")


def shape_of(a_grid, b_grid, Ca, Cb, kernel, stride=1, lda=None, ldb=None, bias=0, linear=0):
    """a_grid / b_grid: (n, D, H, W); padding (k - 1) / 2 — every layer of the path."""
    n, Da, Ha, Wa = a_grid
    _, Db, Hb, Wb = b_grid
    kd, kh, kw = kernel
    return [n, Da, Ha, Wa, Ca, Db, Hb, Wb, Cb, lda or Ca, ldb or Cb, kd, kh, kw, stride, kd // 2, kh // 2, kw // 2, bias, linear]


def query(shape, cus):
    """What the wrappers allocate: the C workspace query for this problem on ``cus`` CUs."""
    lib, s = emu_lib(), shape
    lib.dll.enerf_conv_wgrad_workspace_bytes.restype = lib.dll.enerf_gemm_wgrad_workspace_bytes.restype = C.c_size_t
    with emu_cu_count(lib, cus):
        npos = s[0] * s[1] * s[2] * s[3]
        if s[19]:
            return lib.dll.enerf_gemm_wgrad_workspace_bytes(C.c_longlong(npos), s[4], s[8], s[18])
        return lib.dll.enerf_conv_wgrad_workspace_bytes(C.c_longlong(npos), s[4], s[8], s[11], s[12], s[13])


def route(shape, cus=256, workspace=None, a16=1, b16=1):
    dll = emu_lib().dll
    dll.emu_wgrad_route.restype = C.c_longlong
    dll.emu_wgrad_route.argtypes = [C.POINTER(C.c_int), C.c_int, C.c_int, C.c_longlong, C.c_int, C.c_char_p, C.c_longlong]
    ws = query(shape, cus) if workspace is None else workspace
    buf = C.create_string_buffer(512)
    n = dll.emu_wgrad_route((C.c_int * 20)(*shape), a16, b16, ws, cus, buf, len(buf))
    assert 0 < n <= len(buf)
    lines = buf.raw[:n].decode().splitlines()
    kv = dict(ln.split("=") for ln in lines[1:])
    return Route(lines[0], *[kv[f] if f == "second_stage" else int(kv[f]) for f in Route._fields[1:]])


def grid2(n, H, W, s=1):
    return (n, 1, H, W), (n, 1, H * s, W * s)


def grid3(n, D, H, W, s=1):
    return (n, D, H, W), (n, D * s, H * s, W * s)


# ---- 1. the plan is what gets launched ----------------------------------------------------------------------------------------------
# tag: (entry, a grid (n, D, H, W), Ca, b grid, Cb, k, stride, route at 256 CUs).  a = d y and b = x, except for the transposed layer.
CASES = {
    "gemm_1x1_32_32": ("2d", *grid2(2, 12, 20), 32, 32, 1, 1, "gemm_wgrad<2,2>"),
    "gemm_5_tiles": ("2d", *grid2(2, 12, 20), 80, 8, 1, 1, "conv_wgrad<1,1,1,1,4>"),
    "gemm_entry_bias": ("gemm", (1, 1, 1, 1000), (1, 1, 1, 1000), 40, 24, 1, 1, "gemm_wgrad<3,2>"),
    "c8_8_8": ("2d", *grid2(2, 40, 70), 8, 8, 3, 1, "wgrad2d_3x3_c8<true,true,1>"),
    "c8_32_8": ("2d", *grid2(2, 40, 70), 8, 32, 3, 1, "wgrad2d_3x3_c8<true,true,4>"),
    "c8_16_8": ("2d", *grid2(2, 17, 66), 8, 16, 3, 1, "wgrad2d_3x3_c8<true,true,2>"),
    "c8_3_8": ("2d", *grid2(2, 33, 64), 8, 3, 3, 1, "wgrad2d_3x3_c8<true,false,1>"),
    "c8_8_5": ("2d", *grid2(2, 9, 250), 5, 8, 3, 1, "wgrad2d_3x3_c8<false,true,1>"),
    "p16_16_16": ("2d", *grid2(2, 40, 70), 16, 16, 3, 1, "wgrad2d_3x3_p16<1,1>"),
    "p16_32_16": ("2d", *grid2(2, 33, 45), 16, 32, 3, 1, "wgrad2d_3x3_p16<1,2>"),
    "p16_32_32": ("2d", *grid2(2, 17, 66), 32, 32, 3, 1, "wgrad2d_3x3_p16<2,2>"),
    "3d_16_8": ("3d", *grid3(1, 5, 81, 83), 8, 16, 3, 1, "wgrad3d_c8<true,2>"),
    "3d_32_8_two_columns": ("3d", *grid3(1, 3, 100, 112), 8, 32, 3, 1, "wgrad3d_c8<true,2>"),
    "3d_8_16_swapped": ("3d", *grid3(1, 6, 70, 80), 16, 8, 3, 1, "wgrad3d_c8<true,2>"),
    "3d_32_5_scalar_a": ("3d", *grid3(1, 5, 81, 83), 5, 32, 3, 1, "wgrad3d_c8<false,2>"),
    "generic_64_64": ("3d", *grid3(1, 4, 6, 10), 64, 64, 3, 1, "conv_wgrad<3,3,3,3,2>"),
    "generic_stride2": ("3d", *grid3(1, 2, 3, 5, 2), 16, 8, 3, 2, "conv_wgrad<3,3,3,3,2>"),
    "generic_5x5_stride2": ("2d", *grid2(2, 6, 10, 2), 16, 8, 5, 2, "conv_wgrad<1,5,5,5,1>"),
    "generic_transposed": ("3d", *grid3(1, 2, 3, 5, 2), 64, 32, 3, 2, "conv_wgrad<3,3,3,3,2>"),
}
COLUMNS = {"3d_32_8_two_columns": 2, "3d_32_5_scalar_a": 2}


def case_shape(tag):
    entry, ga, gb, Ca, Cb, k, stride, _ = CASES[tag]
    if entry == "gemm":
        return shape_of(ga, gb, Ca, Cb, (1, 1, 1), bias=1, linear=1)
    return shape_of(ga, gb, Ca, Cb, (3 if entry == "3d" else 1, k, k), stride)


_OPERANDS = {}


def operands(tag):
    if tag not in _OPERANDS:
        _, ga, gb, Ca, Cb = CASES[tag][:5]
        g = torch.Generator().manual_seed(len(_OPERANDS))
        _OPERANDS[tag] = (torch.randn(*ga, Ca, generator=g), torch.randn(*gb, Cb, generator=g))
    return _OPERANDS[tag]


def run_case(lib, tag):
    entry, k, stride = CASES[tag][0], CASES[tag][5], CASES[tag][6]
    a, b = operands(tag)
    if entry == "gemm":
        return lib.gemm_wgrad(a.reshape(-1, a.shape[-1]), b.reshape(-1, b.shape[-1]), bias=True)[0]
    if entry == "2d":
        return lib.conv_wgrad_cl2d(a[:, 0], b[:, 0], k, stride)
    return lib.conv_wgrad_cl(a, b, stride)


def wgrad_launches(rows):
    """[(kernel as rocprofv3 spells it minus the spaces, grid)] of the trace's weight-gradient launches, in order"""
    return [(re.sub(r"[() ]", "", r[1]), r[2]) for r in rows if r[0] == "launch" and re.search(r"wgrad|colsum|k_zero", r[1])]


@pytest.mark.parametrize("cus", [256, 8])
@pytest.mark.parametrize("tag", list(CASES))
def test_predicted_route_is_what_the_entry_launches(tag, cus):
    lib = emu_lib()
    r = route(case_shape(tag), cus)
    assert r.name == CASES[tag][7] and not r.atomic and r.cols == COLUMNS.get(tag, 1), (tag, cus, r)
    with emu_cu_count(lib, cus), emu_trace(lib) as rows:
        run_case(lib, tag)
    got = wgrad_launches(rows)
    assert got == [("k_" + r.name, (r.blocks, r.cols, 1)), ("k_" + r.second_stage, got[1][1])], (tag, cus, r, got)


def test_eight_cus_shrink_the_grids():
    """... so that under 8 CUs the chunk counts drop and the persistent blocks make several passes over their tiles."""
    for tag in ("c8_8_8", "p16_32_32", "3d_32_8_two_columns", "generic_64_64"):       # (the GEMM cases have too few rows for the cap)
        big, small = route(case_shape(tag), 256), route(case_shape(tag), 8)
        assert small.name == big.name and small.chunks < big.chunks and small.scratch_bytes < big.scratch_bytes, (tag, big, small)
    r = route(case_shape("3d_32_8_two_columns"), 8)
    assert r.blocks == 8 and 3 * r.tiles_y * r.tiles_x > 2 * r.blocks, r               # 8 CUs x 2 blocks / 2 columns; 156 tiles


@pytest.mark.parametrize("cus", [256, 8])
def test_without_a_workspace_the_commit_is_atomic(cus):
    """the 16 / 32-channel 3x3x3 layer at 4x6x10 with workspace = NULL: zeroed grad_w, one launch, and the two-stage result at 1e-5"""
    lib = emu_lib()
    g = torch.Generator().manual_seed(5)
    a_cl, b_cl = torch.randn(1, 4, 6, 10, 16, generator=g), torch.randn(1, 4, 6, 10, 32, generator=g)
    shape = shape_of(*grid3(1, 4, 6, 10), 16, 32, (3, 3, 3))
    r = route(shape, cus, workspace=0)
    assert r.name == "conv_wgrad<3,3,3,3,2>" and r.atomic and r.scratch_bytes == 0 and r.second_stage == "", r
    gw = torch.full((16, 32, 3, 3, 3), 7.0)
    with emu_cu_count(lib, cus), emu_trace(lib) as rows:
        two = lib.conv_wgrad_cl(a_cl, b_cl, 1)
        lib._check(lib.dll.enerf_conv_wgrad(a_cl.data_ptr(), b_cl.data_ptr(), 1, 4, 6, 10, 16, 4, 6, 10, 32, 3, 3, 3, 1, 1, 1, 1,
                                            gw.data_ptr(), None, 0, lib.stream_of(a_cl)), "conv_wgrad")
    got = wgrad_launches(rows)[2:]                                     # (after the two-stage call's two launches)
    assert [k for k, _ in got] == ["k_zero", "k_" + r.name] and got[1][1] == (r.blocks, 1, 1), got
    assert float((gw - two).abs().max()) <= 1e-5 * float(two.abs().max())
    # a workspace one byte short of the two-stage form is no workspace
    need = route(shape, cus).scratch_bytes
    assert need == query(shape, cus) and route(shape, cus, workspace=need - 1).atomic and not route(shape, cus, workspace=need).atomic
    # the GEMM has an atomic form too; the tile kernels have none: their layer goes to k_conv_wgrad
    assert route(case_shape("gemm_entry_bias"), workspace=0)[:4] == ("gemm_wgrad<3,2>", 0, 1, "")
    assert route(case_shape("c8_8_8"), workspace=0)[:4] == ("conv_wgrad<1,3,3,3,2>", 0, 1, "")
    assert route(case_shape("3d_16_8"), workspace=0)[:4] == ("conv_wgrad<3,3,3,3,2>", 0, 1, "")


# ---- 2. threshold edges (query only, 256 CUs) ---------------------------------------------------------------------------------------
EDGES = [
    # the 2-D tile from 2048 positions, the 3-D tile from 32768
    (shape_of(*grid2(1, 32, 64), 8, 8, (1, 3, 3)), {}, "wgrad2d_3x3_c8<true,true,1>"),
    (shape_of(*grid2(1, 23, 89), 8, 8, (1, 3, 3)), {}, "conv_wgrad<1,3,3,3,2>"),
    (shape_of(*grid3(1, 8, 64, 64), 8, 16, (3, 3, 3)), {}, "wgrad3d_c8<true,2>"),
    (shape_of(*grid3(1, 7, 31, 151), 8, 16, (3, 3, 3)), {}, "conv_wgrad<3,3,3,3,2>"),
    # the tap split of 3x3x3 below 50000 positions; 5x5 always splits
    (shape_of(*grid3(1, 1, 1, 49999), 64, 64, (3, 3, 3)), {}, "conv_wgrad<3,3,3,3,2>"),
    (shape_of(*grid3(1, 1, 1, 50000), 64, 64, (3, 3, 3)), {}, "conv_wgrad<3,3,3,1,4>"),
    (shape_of(*grid2(1, 10, 10), 16, 8, (1, 5, 5)), {}, "conv_wgrad<1,5,5,5,1>"),
    (shape_of(*grid2(1, 1000, 1000), 16, 8, (1, 5, 5)), {}, "conv_wgrad<1,5,5,5,1>"),
    # 4 x 6 tiles take the GEMM, 5 x 1 and 1 x 7 do not
    (shape_of(*grid2(1, 10, 10), 64, 96, (1, 1, 1)), {}, "gemm_wgrad<4,6>"),
    (shape_of(*grid2(1, 10, 10), 80, 16, (1, 1, 1)), {}, "conv_wgrad<1,1,1,1,4>"),
    (shape_of(*grid2(1, 10, 10), 16, 97, (1, 1, 1)), {}, "conv_wgrad<1,1,1,1,4>"),
    (shape_of(*grid2(1, 10, 10), 64, 95, (1, 1, 1), bias=1, linear=1), {}, "gemm_wgrad<4,6>"),
    (shape_of(*grid2(1, 10, 10), 64, 96, (1, 1, 1), bias=1, linear=1), {}, "conv_wgrad<1,1,1,1,4>"),     # (the bias column is the 97th)
    # a misaligned or ld % 4 != 0 operand: c8 stages it with scalar loads ...
    (shape_of(*grid2(2, 40, 70), 8, 8, (1, 3, 3)), dict(a16=0), "wgrad2d_3x3_c8<false,true,1>"),
    (shape_of(*grid2(2, 40, 70), 8, 8, (1, 3, 3)), dict(b16=0), "wgrad2d_3x3_c8<true,false,1>"),
    (shape_of(*grid2(2, 40, 70), 8, 8, (1, 3, 3), lda=12), {}, "wgrad2d_3x3_c8<true,true,1>"),
    (shape_of(*grid2(2, 40, 70), 8, 8, (1, 3, 3), lda=9), {}, "wgrad2d_3x3_c8<false,true,1>"),
    (shape_of(*grid2(2, 40, 70), 8, 8, (1, 3, 3), ldb=10), {}, "wgrad2d_3x3_c8<true,false,1>"),
    (shape_of(*grid3(1, 5, 81, 83), 8, 16, (3, 3, 3)), dict(a16=0), "wgrad3d_c8<false,2>"),
    (shape_of(*grid3(1, 6, 70, 80), 16, 8, (3, 3, 3)), dict(b16=0), "wgrad3d_c8<false,2>"),               # (swapped: the kernel's A is b)
    # ... and p16, the wide B blocks of c8 and the 3-D B operand have no scalar staging: the generic kernel
    (shape_of(*grid2(2, 40, 70), 16, 16, (1, 3, 3)), dict(a16=0), "conv_wgrad<1,3,3,3,2>"),
    (shape_of(*grid2(2, 40, 70), 16, 16, (1, 3, 3)), dict(b16=0), "conv_wgrad<1,3,3,3,2>"),
    (shape_of(*grid2(2, 40, 70), 16, 16, (1, 3, 3), ldb=18), {}, "conv_wgrad<1,3,3,3,2>"),
    (shape_of(*grid2(2, 40, 70), 8, 32, (1, 3, 3)), dict(b16=0), "conv_wgrad<1,3,3,3,2>"),
    (shape_of(*grid3(1, 5, 81, 83), 8, 16, (3, 3, 3)), dict(b16=0), "conv_wgrad<3,3,3,3,2>"),
    (shape_of(*grid3(1, 5, 81, 83), 8, 16, (3, 3, 3), ldb=18), {}, "conv_wgrad<3,3,3,3,2>"),
    (shape_of(*grid3(1, 6, 70, 80), 16, 8, (3, 3, 3)), dict(a16=0), "conv_wgrad<3,3,3,3,2>"),
    # stride 2 and unequal grids keep 3x3 layers off the tiles; kernels without an instantiation have no route
    (shape_of(*grid2(2, 40, 70, 2), 8, 8, (1, 3, 3), stride=2), {}, "conv_wgrad<1,3,3,3,2>"),
    (shape_of(*grid2(1, 10, 10), 8, 8, (1, 7, 7)), {}, "none"),
    (shape_of(*grid3(1, 4, 10, 10), 8, 8, (3, 1, 1)), {}, "none"),
]


@pytest.mark.parametrize("i", range(len(EDGES)))
def test_threshold_edges(i):
    shape, how, want = EDGES[i]
    r = route(shape, **how)
    assert r.name == want and not r.atomic, (shape, how, r)


# ---- 3. the queries cover the routes ------------------------------------------------------------------------------------------------
CHANNELS = (1, 3, 4, 5, 8, 16, 32, 64, 80)
# (n, D, H, W) with the given number of positions: image-like, one row, one column, and one position per image (the most tiles)
GRIDS = {100: [(1, 1, 10, 10), (1, 4, 5, 5), (100, 1, 1, 1)], 2048: [(1, 1, 32, 64), (2, 4, 8, 32), (1, 1, 2048, 1), (2048, 1, 1, 1)],
         32768: [(1, 1, 128, 256), (1, 8, 64, 64), (1, 1, 1, 32768), (32768, 1, 1, 1)],
         10 ** 6: [(1, 1, 1000, 1000), (1, 10, 250, 400), (1, 1, 10 ** 6, 1), (10 ** 6, 1, 1, 1)]}


def test_query_covers_every_route():
    """enerf_*_wgrad_workspace_bytes >= scratch_bytes of the route taken with that workspace, and that route commits in two stages."""
    shapes = [(case_shape(tag), {}) for tag in CASES] + [(s, how) for s, how, want in EDGES if want != "none"]
    for Ca, Cb, kernel, (npos, grids) in itertools.product(CHANNELS, CHANNELS, ((1, 1, 1), (1, 3, 3), (1, 5, 5), (3, 3, 3)), GRIDS.items()):
        for n, D, H, W in grids:
            if kernel[0] == 1 and D > 1:
                n, D = n * D, 1
            assert n * D * H * W == npos
            shapes.append((shape_of(*grid3(n, D, H, W), Ca, Cb, kernel), {}))
            shapes.append((shape_of(*(grid3 if kernel[0] == 3 else grid2)(*((n, D, H, W) if kernel[0] == 3 else (n, H, W)), 2), Ca, Cb, kernel, stride=2),
                           dict(a16=0, b16=0)))
        shapes.append((shape_of(*grid2(1, 1, npos), Ca, Cb, (1, 1, 1), bias=1, linear=1), {}))
        shapes.append((shape_of(*grid2(1, 1, npos), Ca, Cb, (1, 1, 1), lda=Ca + 3, linear=1), {}))
    for cus in (8, 256):
        for shape, how in shapes:
            ws = query(shape, cus)
            r = route(shape, cus, workspace=ws, **how)
            assert r.name != "none" and not r.atomic and 0 < r.scratch_bytes <= ws, (shape, how, cus, ws, r)


# ---- 4. the training step's routes are the parent's ---------------------------------------------------------------------------------
def training_layers():
    """(name, shape) of every convolution whose weight gradient the bench's training step takes (bench.py --train: EnerfConfig(), one
    512x640 sample with three source views), from the networks' own modules: FeatureNetTrainFn / CostRegTrainFn of autograd.py."""
    from enerf_amd.config import EnerfConfig
    from enerf_amd.network import CostRegParams, FeatureNet
    cas, H, W, S = EnerfConfig().cas, 512, 640, 3
    out = []
    fnet = FeatureNet()
    div = {"conv0": 1, "conv1": 2, "conv2": 4, "toplayer": 4, "lat1": 2, "lat0": 1, "smooth1": 2, "smooth0": 1}       # output resolution
    for name, m in fnet.named_modules():
        if not isinstance(m, torch.nn.Conv2d):
            continue
        k, s, d = m.kernel_size[0], m.stride[0], div[name.split(".")[0]]
        a, b = (S, 1, H // d, W // d), (S, 1, H // d * s, W // d * s)
        if k == 1 and s == 1 and m.bias is not None:                  # enerf_gemm_wgrad with the bias column
            out.append((name, shape_of((1, 1, 1, S * a[2] * a[3]), (1, 1, 1, S * a[2] * a[3]), m.out_channels, m.in_channels, (1, 1, 1), bias=1, linear=1)))
        else:
            out.append((name, shape_of(a, b, m.out_channels, m.in_channels, (1, k, k), s)))
    for lvl in range(cas.num):
        net = CostRegParams((32, 16)[lvl], lvl != 0)
        D, h, w = cas.volume_planes[lvl], int(H * cas.volume_scale[lvl]), int(W * cas.volume_scale[lvl])
        div = 1                                                       # of the layer's INPUT grid
        for name, m in net.named_modules():
            if isinstance(m, torch.nn.ConvTranspose3d):               # a = x on the coarse grid, b = d y on the fine one
                out.append((f"l{lvl}.{name}", shape_of((1, D // div, h // div, w // div), (1, 2 * D // div, 2 * h // div, 2 * w // div),
                                                       m.in_channels, m.out_channels, (3, 3, 3), 2)))
                div //= 2
            elif isinstance(m, torch.nn.Conv3d) and "depth_conv" not in name and "feat_conv" not in name:
                s = m.stride[0]
                out.append((f"l{lvl}.{name}", shape_of((1, D // div // s, h // div // s, w // div // s), (1, D // div, h // div, w // div),
                                                       m.out_channels, m.in_channels, (3, 3, 3), s)))
                div *= s
        assert div == 1
        out.append((f"l{lvl}.heads", shape_of(*grid3(1, D, h, w), 16, 8, (3, 3, 3))))       # feat_conv ++ depth_conv as one 8 -> 16 layer
    return out


def traced_wgrad_kernels():
    """rows of the parent's table for k_conv_wgrad*, k_wgrad2d*, k_wgrad3d* and the single k_gemm_wgrad<...>, per training step (the
    level-1 MLP backward kernel runs once per step)"""
    n, steps = collections.Counter(), 0
    with open(os.path.join(PROFILES, "wgrad_route_refactor_kernels_parent.csv")) as f:
        for row in csv.DictReader(f):
            m = re.match(r"void enerf::(k_(?:conv_wgrad|wgrad2d\w*|wgrad3d\w*|gemm_wgrad)<[^>]*>)\(", row["kernel"])
            if m:
                n[m.group(1).replace(" ", "")] += int(row["calls"])
            if row["kernel"].startswith("void enerf::k_mlp_bwd<3"):
                steps += int(row["calls"])
    assert steps > 0 and all(c % steps == 0 for c in n.values()), (steps, n)
    return collections.Counter({k: c // steps for k, c in n.items()})


def test_training_step_routes_are_the_parent_trace():
    layers = training_layers()
    assert len(layers) == 11 + 8 + 11                 # FeatureNet, MinCostRegNet (level 0), CostRegNet (level 1)
    routes = {name: route(shape) for name, shape in layers}
    assert not any(r.atomic or r.name == "none" for r in routes.values()), routes
    assert collections.Counter("k_" + r.name for r in routes.values()) == traced_wgrad_kernels(), {k: r.name for k, r in routes.items()}
    pinned = {"conv0.0.conv": "wgrad2d_3x3_c8<true,false,1>", "conv0.1.conv": "wgrad2d_3x3_c8<true,true,1>", "conv1.0.conv": "conv_wgrad<1,5,5,5,1>",
              "conv1.1.conv": "wgrad2d_3x3_p16<1,1>", "conv2.1.conv": "wgrad2d_3x3_p16<2,2>", "toplayer": "gemm_wgrad<2,3>", "lat1": "gemm_wgrad<2,2>",
              "lat0": "gemm_wgrad<2,1>", "smooth1": "wgrad2d_3x3_p16<1,2>", "smooth0": "wgrad2d_3x3_c8<true,true,4>",
              "l0.conv0.conv": "wgrad3d_c8<true,2>", "l1.conv0.conv": "wgrad3d_c8<true,2>", "l0.heads": "wgrad3d_c8<true,2>",
              "l0.conv1.conv": "conv_wgrad<3,3,3,3,2>", "l1.conv1.conv": "conv_wgrad<3,3,3,1,4>", "l1.conv2.conv": "conv_wgrad<3,3,3,1,4>",
              "l1.conv11.0": "conv_wgrad<3,3,3,1,4>", "l1.conv6.conv": "conv_wgrad<3,3,3,3,2>"}
    assert {k: routes[k].name for k in pinned} == pinned
