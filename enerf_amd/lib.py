"""ctypes binding of the C ABI in include/enerf_hip.h (libenerf_hip.so).

PyTorch is used only as the owner of device memory and streams: every call passes raw
``tensor.data_ptr()`` addresses, sizes and the current HIP stream handle.  There is NO CPU or eager
fallback: if the shared library is missing or a call fails, an exception is raised.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import os
import threading
from typing import Optional

import torch

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_PKG, "libenerf_hip.so")
ABI_VERSION = 11

_f = C.c_void_p     # device float*
_i = C.c_int
_ll = C.c_longlong
_fl = C.c_float


class ConvBn(C.Structure):
    _fields_ = [("w", _f), ("bn_weight", _f), ("bn_bias", _f), ("bn_mean", _f), ("bn_var", _f)]


class CostRegRaw(C.Structure):
    _fields_ = [("conv", ConvBn * 12), ("feat_conv_w", _f), ("depth_conv_w", _f), ("in_channels", _i), ("full", _i)]


class FeatNetRaw(C.Structure):
    _fields_ = [("conv", ConvBn * 6)] + [(n, _f) for n in ("toplayer_w", "toplayer_b", "lat1_w", "lat1_b", "lat0_w",
                                                            "lat0_b", "smooth1_w", "smooth1_b", "smooth0_w", "smooth0_b")]


class NerfRaw(C.Structure):
    _fields_ = [(n, _f) for n in ("view_w", "view_b", "glob_w", "glob_b", "aggw_w", "aggw_b", "fc_w", "fc_b",
                                  "lr0_w", "lr0_b", "sigma_w", "sigma_b", "col0_w", "col0_b", "col2_w", "col2_b")]


class Options(C.Structure):
    """``enerf_options_t``: explicit kernel-variant choices, passed per call (all zero = defaults)."""
    _fields_ = [("conv3d_global_only", _i), ("conv3d_lds_min_voxels", _ll), ("conv3d_pk8", _i),
                ("featnet_unfused", _i), ("featnet_smooth0_plain", _i), ("conv3d_b4", _i), ("single_stream", _i),
                ("side_gate", _i), ("fuse_depth_prep", _i), ("conv3d_t2_variant", _i), ("conv3d_small_variant", _i),
                ("render_precision", _i), ("heads_keep_feat", _i)]

    def __repr__(self):
        return "Options(" + ", ".join(f"{n}={getattr(self, n)}" for n, _ in self._fields_ if getattr(self, n)) + ")"


# what "most frames per second" prefers over "one frame as fast as possible" (enerf_amd/pipeline.py)
def throughput_options() -> "Options":
    # frames in flight already fill the chip: the in-frame side lanes add nothing there (measured equal) and triple the
    # number of streams the runtime has to map onto its few hardware queues
    return Options(single_stream=1)


def _opt(o):
    return None if o is None else C.byref(o)


class MlpBwdArgs(C.Structure):
    """``enerf_mlp_bwd_args_t``."""
    _fields_ = ([(n, _f) for n in ("vox", "x", "g_raw", "packed", "bimg", "g_vox", "g_x")] + [("save", C.c_void_p * 16),
                ("P", _ll), ("F", _i), ("S", _i), ("image_offsets", _i * 8)])


class GatherArgs(C.Structure):
    """``enerf_gather_args_t``."""
    _fields_ = ([(n, _f) for n in ("xyz", "dn", "uv", "tex", "vol", "cam", "tcen", "x", "vox", "g_x", "g_vox", "g_tex",
                                   "g_vol", "g_xyz", "g_dn")]
                + [("P", _ll)] + [(n, _i) for n in ("B", "S", "F", "Hr", "Wr", "D", "h", "w", "ray_w", "n_samples")])


class GemmWgradDesc(C.Structure):
    _fields_ = [("a", _f), ("lda", _i), ("Ca", _i), ("b", _f), ("ldb", _i), ("Cb", _i), ("P", _ll), ("grad_w", _f), ("ldw", _i),
                ("grad_bias", _f), ("partials", _f), ("partial_chunks", _i)]


class RenderArgs(C.Structure):
    _fields_ = ([(n, _f) for n in ("rays12", "tex", "vol", "src_exts", "src_ixts", "tar_ext", "packed", "rgb",
                                   "depth", "weights")]
                + [(n, _i) for n in ("B", "N", "S", "n_samples", "depth_inv", "Hr", "Wr", "F", "D", "h", "w",
                                     "white_bkgd")]
                + [("render_scale", _fl)]
                + [(n, _f) for n in ("rays8", "depth_map", "std_map", "nf_map")] + [("map_h", _i), ("map_w", _i)]
                + [("options", C.POINTER(Options)), ("ray_index", C.c_void_p), ("ray_count", C.c_void_p),
                   ("scatter_rgb", _i), ("max_blocks", _i)])


class RenderRawArgs(C.Structure):
    """``enerf_render_raw_args_t``."""
    _fields_ = ([(n, _f) for n in ("rays12", "rays8", "depth_map", "std_map", "nf_map")] + [("map_h", _i), ("map_w", _i)]
                + [(n, _f) for n in ("tex", "vol", "src_exts", "src_ixts", "tar_ext", "packed", "raw", "z")]
                + [(n, _i) for n in ("B", "N", "S", "n_samples", "depth_inv", "Hr", "Wr", "F", "D", "h", "w")]
                + [("render_scale", _fl), ("ray_index", C.c_void_p), ("ray_count", C.c_void_p), ("max_blocks", _i)])


MAX_FG_LAYERS = 4


class CompositeLayersArgs(C.Structure):
    """``enerf_composite_layers_t``."""
    _fields_ = ([("fg_raw", C.c_void_p * MAX_FG_LAYERS), ("fg_z", C.c_void_p * MAX_FG_LAYERS), ("win", (_i * 4) * MAX_FG_LAYERS),
                 ("bg_raw", _f), ("bg_z", _f)] + [(n, _i) for n in ("L", "Ns", "H", "W", "white_bkgd")]
                + [(n, _f) for n in ("rgb", "depth", "weights", "net_output", "z_vals")])


class CompositeLayersBwdArgs(C.Structure):
    """``enerf_composite_layers_bwd_t``."""
    _fields_ = [("fwd", CompositeLayersArgs), ("grad_rgb", _f), ("grad_depth", _f), ("grad_weights", _f),
                ("grad_fg_raw", C.c_void_p * MAX_FG_LAYERS), ("grad_bg_raw", _f)]


MAX_LEVELS = 3
STAGE_COUNT = 2 + 6 * MAX_LEVELS
STAGE_NAMES = ["begin", "feature_net"] + [f"{n}_{i}" for i in range(MAX_LEVELS)
                                          for n in ("prep", "volume", "cost_reg", "depth_reg", "texels", "render")]
_dL, _iL, _fL = C.c_double * MAX_LEVELS, C.c_int * MAX_LEVELS, C.c_void_p * MAX_LEVELS


class Cascade(C.Structure):
    """``enerf_cascade_t`` (cfg.enerf.cas_config)."""
    _fields_ = [("num", _i), ("depth_inv", _iL), ("volume_scale", _dL), ("volume_planes", _iL), ("im_feat_scale", _dL),
                ("im_ibr_scale", _dL), ("render_scale", _dL), ("render_im_feat_level", _iL), ("nerf_model_feat_ch", _iL),
                ("render_if", _iL), ("num_samples", _iL), ("white_bkgd", _i)]


class FrameArgs(C.Structure):
    """``enerf_frame_args_t``."""
    _fields_ = ([(n, _f) for n in ("src_inps", "src_exts", "src_ixts", "tar_ext", "tar_ixt", "near_far")]
                + [("rays", _fL), ("n_rays", _iL), ("mask_at_box", C.c_void_p), ("mask_elem_bytes", _i)]
                + [(n, _i) for n in ("B", "S", "H", "W")] + [("cas", Cascade)]
                + [("feature_net_packed", _f), ("cost_reg_packed", _fL), ("nerf_packed", _fL), ("feats_nchw", C.c_void_p * 3)]
                + [(n, _fL) for n in ("rgb", "depth", "weights", "depth_mvs", "std")]
                + [("ray_index", C.c_void_p), ("ray_count", C.c_void_p), ("ray_index_ready", _i),
                   ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t), ("options", C.POINTER(Options)),
                   ("stage_events", C.POINTER(C.c_void_p))])


_CASC = MAX_FG_LAYERS + 1           # cascades of a composite frame: the foreground layers, then the background


class CompositePrepArgs(C.Structure):
    """``enerf_composite_prep_t``."""
    _fields_ = ([(n, _f) for n in ("src_ixts", "src_exts", "tar_ixt", "tar_ext", "near_far")] + [("L", _i), ("S", _i), ("num_levels", _i)]
                + [("src_scale", _fl * MAX_LEVELS), ("tar_scale", _fl * MAX_LEVELS), ("proj", _fL)]
                + [(n, _i) for n in ("fg_planes", "bg_planes", "h", "w", "depth_inv")]
                + [("dv", C.c_void_p * _CASC), ("nf", C.c_void_p * _CASC), ("Hr", _iL), ("Wr", _iL),
                   ("win", ((_i * 4) * MAX_FG_LAYERS) * MAX_LEVELS), ("index", (C.c_void_p * MAX_FG_LAYERS) * MAX_LEVELS),
                   ("count", (C.c_void_p * MAX_FG_LAYERS) * MAX_LEVELS)])


class CompositeFrameArgs(C.Structure):
    """``enerf_composite_frame_args_t``."""
    _fields_ = ([(n, _f) for n in ("src_inps", "bg_src_inps", "src_exts", "src_ixts", "tar_ext", "tar_ixt", "near_far")]
                + [("bbox", (_fl * 4) * MAX_FG_LAYERS)] + [(n, _i) for n in ("L", "S", "H", "W")] + [("cas", Cascade)]
                + [("bg_volume_planes", _iL), ("rays", _fL), ("feature_net_packed", _f), ("feature_net_bg_packed", _f),
                   ("cost_reg_packed", (C.c_void_p * _CASC) * MAX_LEVELS), ("nerf_packed", (C.c_void_p * _CASC) * MAX_LEVELS)]
                + [(n, _fL) for n in ("rgb", "depth", "weights", "net_output", "z_vals")]
                + [("depth_map", (C.c_void_p * _CASC) * MAX_LEVELS), ("std_map", (C.c_void_p * _CASC) * MAX_LEVELS),
                   ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t), ("options", C.POINTER(Options))])


class SourceCacheStruct(C.Structure):
    """``enerf_source_cache_t``."""
    _fields_ = ([(n, _f) for n in ("feat_l0", "feat_l1", "feat_l2")] + [("tex", _fL), ("exts", _f), ("ixts", _f)]
                + [(n, _i) for n in ("V", "H", "W", "l2_stride")])


SOURCE_CACHE_BUFFERS = 5 + MAX_LEVELS


class CompositeCacheStruct(C.Structure):
    """``enerf_composite_cache_t``."""
    _fields_ = ([(n, _fL) for n in ("fg_feat", "fg_tex", "bg_feat", "bg_tex")] + [("exts", _f), ("ixts", _f)]
                + [(n, _i) for n in ("V", "H", "W")])


COMPOSITE_CACHE_BUFFERS = 4 * MAX_LEVELS + 2
VHULL_MAX_VIEWS = 64


class VhullArgs(C.Structure):
    """``enerf_vhull_t``."""
    _fields_ = ([("masks", C.c_void_p), ("exts", _f), ("ixts", _f)] + [(n, _i) for n in ("V", "H", "W")]
                + [("scene_bounds", (_fl * 3) * 2), ("grid", _i * 3)] + [(n, _i) for n in ("n_layers", "labels", "min_views", "max_miss")]
                + [("pad", C.c_double), ("bounds", _f), ("counts", C.c_void_p), ("flags", C.c_void_p), ("corners", _f),
                   ("occupancy", C.c_void_p), ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t)])


class _ConvWB(C.Structure):
    _fields_ = [("w", _f), ("b", _f)]


class LpipsRaw(C.Structure):
    """``enerf_lpips_raw_t``."""
    _fields_ = [("conv", _ConvWB * 13), ("lin", _f * 5)]


class PerceptualRaw(C.Structure):
    """``enerf_perceptual_raw_t``."""
    _fields_ = [("conv", _ConvWB * 10)]


# the VGG16 trunk of LPIPS: (cin, cout) of features.{0,2,5,7,10,12,14,17,19,21,24,26,28}, the tap widths, the rect modes
VGG_CONVS = ((3, 64), (64, 64), (64, 128), (128, 128), (128, 256), (256, 256), (256, 256), (256, 512), (512, 512), (512, 512),
             (512, 512), (512, 512), (512, 512))
LPIPS_TAP_CHANNELS = (64, 128, 256, 512, 512)
RECT_NONE, RECT_CROP, RECT_XYWH = 0, 1, 3
PERCEPTUAL_CONVS = VGG_CONVS[:10]          # features[:23]: the trainer's perceptual term stops after relu4_3


def cascade_struct(cfg) -> Cascade:
    """EnerfConfig -> enerf_cascade_t."""
    cas = cfg.cas
    if cas.num > MAX_LEVELS:
        raise EnerfError(f"cas_config.num={cas.num} > {MAX_LEVELS}")
    c = Cascade(num=cas.num, white_bkgd=int(cfg.white_bkgd))
    for i in range(cas.num):
        c.depth_inv[i] = int(cas.depth_inv[i]); c.volume_scale[i] = float(cas.volume_scale[i])
        c.volume_planes[i] = int(cas.volume_planes[i]); c.im_feat_scale[i] = float(cas.im_feat_scale[i])
        c.im_ibr_scale[i] = float(cas.im_ibr_scale[i]); c.render_scale[i] = float(cas.render_scale[i])
        c.render_im_feat_level[i] = int(cas.render_im_feat_level[i])
        c.nerf_model_feat_ch[i] = int(cas.nerf_model_feat_ch[i]); c.render_if[i] = int(cas.render_if[i])
        c.num_samples[i] = int(cas.num_samples[i])
    return c


_SIGNATURES = {
    "enerf_abi_version": (_i, []),
    "enerf_last_error": (C.c_char_p, []),
    "enerf_channels_last": (_i, [_f, _f, _i, _i, _ll, _i, _f]),
    "enerf_channels_first": (_i, [_f, _f, _i, _i, _ll, _i, _f]),
    "enerf_pack_img_feat_rgb": (_i, [_f, _i, _i, _i, _f, _i, _i, _i, _i, _i, _i, _f, _f]),
    "enerf_feature_net_packed_floats": (_ll, []),
    "enerf_feature_net_pack": (_i, [C.POINTER(FeatNetRaw), _f, _f]),
    "enerf_feature_net_workspace_bytes": (C.c_size_t, [_i, _i, _i]),
    "enerf_feature_net": (_i, [_f, _f, _i, _i, _i, _f, _f, _f, _i, _f, C.c_size_t, C.POINTER(Options), _f]),
    "enerf_feature_net_stage": (_i, [_f, _f, _i, _i, _i, _f, _f, _f, _i, _f, C.c_size_t, _i, C.POINTER(Options), _f]),
    "enerf_pack_texels_cl": (_i, [_f, _i, _f, _i, _i, _i, _i, _i, _i, _f, _f]),
    "enerf_get_proj_mats": (_i, [_f, _f, _f, _f, _i, _i, _fl, _fl, _f, _f]),
    "enerf_get_depth_values": (_i, [_f, _f, _f, _f, _i, _i, _i, _i, _i, _i, _i, _f, _f, _f]),
    "enerf_level_prep": (_i, [_f, _f, _f, _f, _i, _i, _fl, _fl, _f, _f, _f, _f, _f, _i, _i, _i, _i, _i, _i, _f, _f, _f]),
    "enerf_build_feature_volume": (_i, [_f, _f, _f, _i, _i, _i, _i, _i, _i, _i, _i, _f, _f]),
    "enerf_cost_reg_packed_floats": (_ll, [_i, _i]),
    "enerf_cost_reg_pack": (_i, [C.POINTER(CostRegRaw), _f, _f]),
    "enerf_cost_reg_workspace_bytes": (C.c_size_t, [_i, _i, _i, _i, _i]),
    "enerf_cost_reg": (_i, [_f, _i, _i, _f, _i, _i, _i, _i, _f, _f, _f, C.c_size_t, C.POINTER(Options), _f]),
    "enerf_cost_reg_prob": (_i, [_f, _i, _i, _f, _i, _i, _i, _i, _f, _f, C.c_size_t, C.POINTER(Options), _f]),
    "enerf_depth_regression": (_i, [_f, _f, _i, _i, _i, _i, _i, _f, _f, _f]),
    "enerf_build_rays": (_i, [_f, _f, _f, _f, _i, _i, _i, _i, _i, _i, _i, _f, _f]),
    "enerf_nerf_packed_floats": (_ll, [_i]),
    "enerf_nerf_pack": (_i, [C.POINTER(NerfRaw), _i, _i, _f, _f]),
    "enerf_render_rays": (_i, [C.POINTER(RenderArgs), _f]),
    "enerf_mask_compact_workspace_bytes": (C.c_size_t, [_ll]),
    "enerf_mask_compact": (_i, [C.c_void_p, _i, _ll, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, _f]),
    "enerf_forward_workspace_bytes": (C.c_size_t, [C.POINTER(FrameArgs)]),
    "enerf_forward": (_i, [C.POINTER(FrameArgs), _f]),
    "enerf_build_feature_volume_bwd": (_i, [_f, _f, _f, _f, _i, _i, _i, _i, _i, _i, _i, _i, _f, _f, _f]),
    "enerf_depth_regression_bwd": (_i, [_f, _f, _f, _f, _i, _i, _i, _i, _i, _f, _f, _f]),
    "enerf_conv_wgrad_workspace_bytes": (C.c_size_t, [_ll, _i, _i, _i, _i, _i]),
    "enerf_conv_wgrad": (_i, [_f, _f] + [_i] * 16 + [_f, C.c_void_p, C.c_size_t, _f]),
    "enerf_gemm_wgrad_workspace_bytes": (C.c_size_t, [_ll, _i, _i, _i]),
    "enerf_nerf_mlp_bwd": (_i, [C.POINTER(MlpBwdArgs), _f]),
    "enerf_nerf_mlp_bwd_chunks": (_ll, [_ll]),
    "enerf_nerf_mlp_bwd_partials": (_i, [C.POINTER(MlpBwdArgs), _i, _f, _f, _f, _f, _f]),
    "enerf_colsum": (_i, [_f, _i, _i, _f, _f]),
    "enerf_gemm_wgrad": (_i, [_f, _i, _i, _f, _i, _i, _ll, _f, _f, C.c_void_p, C.c_size_t, _f]),
    "enerf_bn_train_apply": (_i, [_f, _ll, _i, C.c_void_p, C.c_size_t, _f, _f, C.c_double, C.c_double, _f, _f, C.c_void_p, _i, C.c_void_p, _f, _f, _i, _f, _f]),
    "enerf_bn_train_bwd_apply": (_i, [_f, _f, _i, _ll, _i, C.c_void_p, C.c_size_t, C.c_void_p, _f, _f, _f, _f]),
    "enerf_wgrad_reduce_begin": (_i, []),
    "enerf_wgrad_reduce_flush": (_i, [_f]),
    "enerf_selftest_checks": (_i, []),
    "enerf_selftest_primitives": (_i, [_f, _i, _f, _i, C.c_void_p, _f]),
    "enerf_gemm_wgrad_group_workspace_bytes": (C.c_size_t, [C.POINTER(GemmWgradDesc), _i]),
    "enerf_gemm_wgrad_group": (_i, [C.POINTER(GemmWgradDesc), _i, C.c_void_p, C.c_size_t, _f]),
    "enerf_nerf_mlp_fwd": (_i, [_f, _f, _f, _ll, _i, _i, _f, _f]),
    "enerf_gather_fwd": (_i, [C.POINTER(GatherArgs), _f]),
    "enerf_gather_bwd": (_i, [C.POINTER(GatherArgs), _f]),
    "enerf_conv3d_layer_packed_floats": (_ll, [_i, _i, _i]),
    "enerf_conv3d_layer_pack": (_i, [_f, _i, _i, _i, _f, _f]),
    "enerf_conv3d_layer": (_i, [_f, _i, _i, _i, _f, _f, _f, _i, _i, _i, _i, C.POINTER(Options), _f]),
    "enerf_up2_adjoint": (_i, [_f, _f, _i, _i, _i, _i, _f, _f]),
    "enerf_conv2d_layer_packed_floats": (_ll, [_i, _i, _i]),
    "enerf_conv2d_layer_pack": (_i, [_f, _f, _i, _i, _i, _f, _f]),
    "enerf_conv2d_layer": (_i, [_f, _i, _i, _i, _i, _f, _f, _f, _i, _i, _i, _f]),
    "enerf_channel_sums": (_i, [_f, _f, _f, _f, _f, _ll, _i, C.c_void_p, _f]),
    "enerf_channel_sums_workspace_bytes": (C.c_size_t, [_ll, _i]),
    "enerf_channel_sums_ws": (_i, [_f, _f, _f, _f, _f, _ll, _i, C.c_void_p, C.c_void_p, C.c_size_t, _f]),
    "enerf_bn_train_coeffs": (_i, [C.c_void_p, C.c_void_p, C.c_double, _f, _f, C.c_double, C.c_double, _f, _f, C.c_void_p, _i, _i,
                                   C.c_void_p, _f, _f]),
    "enerf_bn_train_bwd_coeffs": (_i, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p, _f, _i, _f, _f, _f]),
    "enerf_bn_train_stats": (_i, [_f, _ll, _i, C.c_void_p, C.c_size_t, _f, _f, C.c_double, C.c_double, _f, _f, C.c_void_p, _i, C.c_void_p,
                                  C.c_void_p, _f, C.c_void_p]),
    "enerf_bn_train_bwd_stats": (_i, [_f, _f, _f, _f, _f, _ll, _i, C.c_void_p, C.c_size_t, C.c_void_p, _f, _f, _f, C.c_void_p]),
    "enerf_channel_affine": (_i, [_f, _f, _f, _f, _f, _f, _f, _f, _f, _i, _ll, _i, _f, _f]),
    "enerf_conv2d_s2k5_dgrad_workspace_bytes": (C.c_size_t, [_i, _i, _i, _i, _i]),
    "enerf_conv2d_s2k5_dgrad": (_i, [_f, _i, _i, _f, _f, _f, _i, _i, _i, C.c_void_p, C.c_size_t, _f]),
    "enerf_conv2d_s2k5_dgrad_packed_floats": (_ll, [_i, _i]),
    "enerf_conv2d_s2k5_dgrad_pack": (_i, [_f, _i, _i, _f, _f, _f]),
    "enerf_conv2d_s2k5_dgrad_packed": (_i, [_f, _i, _i, _f, _f, _f, _i, _i, _i, C.c_void_p, C.c_size_t, _f]),
    "enerf_resize_ac_adjoint": (_i, [_f, _f, _i, _i, _i, _i, _i, _f, _f]),
    "enerf_get_depth_values_bwd": (_i, [_f, _f, _f, _f, _i, _i, _i, _i, _i, _i, _i, _f, _f, _f, _f]),
    "enerf_ray_samples_fwd": (_i, [_f, _f, _f, _f, _i, _i, _i, _i, _i, _i, _i, _i, _f, _f, _f, _f, _f, _f]),
    "enerf_ray_samples_bwd": (_i, [_f, _f, _f, _f, _f, _f, _i, _i, _i, _i, _i, _i, _i, _i, _f, _f, _f]),
    "enerf_camera_tables": (_i, [_f, _f, _f, _i, _i, _fl, _f, _f, _f]),
    "enerf_weights_flip_transpose": (_i, [_f, _i, _i, _i, _f, _f]),
    "enerf_concat2_pad": (_i, [_f, _ll, _f, _ll, _ll, _f, _f]),
    "enerf_pack_texels_train": (_i, [_f, _i, _f, _i, _i, _i, _i, _i, _f, _f]),
    "enerf_slice_channels": (_i, [_f, _ll, _i, _i, _i, _f, _f]),
    "enerf_concat_channels": (_i, [_f, _i, _f, _i, _ll, _i, _f, _f]),
    "enerf_gather_images": (_i, [C.c_void_p, _i, C.c_void_p, C.c_void_p, _ll, _f, _f]),
    "enerf_add": (_i, [_f, _f, _ll, _f, _f]),
    "enerf_cast_f64_f32": (_i, [C.c_void_p, _ll, _f, _f]),
    "enerf_reciprocal": (_i, [_f, _ll, _f, _f]),
    "enerf_composite": (_i, [_f, _f, _ll, _i, _i, _f, _f, _f, _f]),
    "enerf_composite_bwd": (_i, [_f, _f, _f, _f, _f, _ll, _i, _f, _f, _f]),
    "enerf_gen_rays": (_i, [_f, _f, _i, _i, _i, _fl, _f, _f]),
    "enerf_pack_rgb8": (_i, [_f, _i, _i, _i, _f, _f]),
    "enerf_eval_stats": (_i, [_f, _f, C.c_void_p, _i, _ll, _i, _i, _i, _i, _f, _f, _ll, _f, _f]),
    "enerf_eval_ssim_workspace_bytes": (C.c_size_t, [_i, _i, _i, _i, _i, _i]),
    "enerf_eval_ssim": (_i, [_f, _f, C.c_void_p, _i, _i, _i, _i, _i, _i, _i, _i, C.c_void_p, C.c_void_p, _f]),
    "enerf_lpips_packed_floats": (_ll, []),
    "enerf_lpips_pack": (_i, [C.POINTER(LpipsRaw), _f, _f]),
    "enerf_eval_lpips_workspace_bytes": (C.c_size_t, [_i] * 8),
    "enerf_eval_lpips": (_i, [_f, _f, _f, C.c_void_p, _i, _i] + [_i] * 8 + [C.c_void_p, C.c_size_t, C.c_void_p, _f]),
    "enerf_lpips_front": (_i, [_f, _f, _f, C.c_void_p, _i, _i] + [_i] * 8 + [_f, _f]),
    "enerf_vgg_conv3x3_packed_floats": (_ll, [_i, _i]),
    "enerf_vgg_conv3x3_pack": (_i, [_f, _f, _i, _i, _f, _f]),
    "enerf_vgg_conv3x3": (_i, [_f, _i, _i, _f, _f, _i, _i, _i, _i, _f]),
    "enerf_mask_bbox": (_i, [C.c_void_p, _i, _i, _i, _i, _i, C.c_void_p, _f]),
    "enerf_perceptual_packed_floats": (_ll, []),
    "enerf_perceptual_pack": (_i, [C.POINTER(PerceptualRaw), _f, _f]),
    "enerf_perceptual_workspace_bytes": (C.c_size_t, [_i, _i, _i]),
    "enerf_perceptual_layout": (_i, [_i, _i, _i, C.POINTER(_ll)]),
    "enerf_perceptual_fwd": (_i, [_f, _f, _f, _i, _i, _i, C.c_void_p, C.c_size_t, C.c_void_p, _f]),
    "enerf_perceptual_bwd": (_i, [_f, _i, _i, _i, C.c_void_p, C.c_size_t, _f, _f, _f]),
    "enerf_vgg_conv3x3_dgrad_packed_floats": (_ll, [_i, _i]),
    "enerf_vgg_conv3x3_dgrad_pack": (_i, [_f, _i, _i, _f, _f]),
    "enerf_vgg_conv3x3_dgrad": (_i, [_f, _i, _i, _f, _f, _i, _i, _i, _f]),
    "enerf_gen_rays_at": (_i, [_f, _f, C.c_void_p, _i, _i, _fl, _f, _f]),
    "enerf_rays_bbox_mask": (_i, [_f, _f, _ll, C.c_void_p, _f]),
    "enerf_select_views": (_i, [_f, _i, _f, _i, C.c_void_p, _f]),
    "enerf_gather_views": (_i, [_f, _f, _f, C.c_void_p, _i, _i, _i, _f, _f, _f, _f]),
    "enerf_source_cache_sizes": (_i, [C.POINTER(Cascade), _i, _i, _i, C.POINTER(_i), C.POINTER(_ll)]),
    "enerf_source_cache_build_workspace_bytes": (C.c_size_t, [_i, _i]),
    "enerf_source_cache_build": (_i, [C.POINTER(SourceCacheStruct), _f, _f, _f, _f, C.POINTER(Cascade), _i, C.c_void_p, C.c_size_t,
                                      C.POINTER(Options), _f]),
    "enerf_forward_cached_workspace_bytes": (C.c_size_t, [C.POINTER(FrameArgs), C.POINTER(SourceCacheStruct)]),
    "enerf_forward_cached": (_i, [C.POINTER(FrameArgs), C.POINTER(SourceCacheStruct), C.c_void_p, _f]),
    "enerf_ingest_views_u8": (_i, [C.c_void_p, C.c_void_p, _i, _i, _i, _i, _f, _f]),
    "enerf_ingest_raw_u8": (_i, [C.c_void_p, C.c_void_p, _f, _f, _i, _i, _i, C.c_double, _i, _i, _i, _i, _i, C.c_void_p, _f, C.c_void_p, _f]),
    "enerf_ingest_raw_geometry": (_i, [_i, _i, C.c_double, C.POINTER(_i), C.POINTER(_i)]),
    "enerf_bounds_near_far": (_i, [_f, _i, _f, _i, _fl, _f, _f]),
    "enerf_build_feature_volume_window": (_i, [_f, _f, _f] + [_i] * 12 + [_f, _f]),
    "enerf_depth_regression_window": (_i, [_f, _f] + [_i] * 9 + [_f, _f, _f]),
    "enerf_window_ray_index": (_i, [_i] * 6 + [C.c_void_p, C.c_void_p, _f]),
    "enerf_render_rays_raw": (_i, [C.POINTER(RenderRawArgs), _f]),
    "enerf_composite_layers": (_i, [C.POINTER(CompositeLayersArgs), _f]),
    "enerf_build_feature_volume_window_bwd": (_i, [_f, _f, _f, _f] + [_i] * 12 + [_f, _f, _f]),
    "enerf_depth_regression_window_bwd": (_i, [_f, _f, _f, _f] + [_i] * 9 + [_f, _f, _f]),
    "enerf_composite_layers_bwd": (_i, [C.POINTER(CompositeLayersBwdArgs), _f]),
    "enerf_composite_prep": (_i, [C.POINTER(CompositePrepArgs), _f]),
    "enerf_forward_composite_workspace_bytes": (C.c_size_t, [C.POINTER(CompositeFrameArgs)]),
    "enerf_forward_composite": (_i, [C.POINTER(CompositeFrameArgs), _f]),
    "enerf_composite_cache_sizes": (_i, [C.POINTER(Cascade), _i, _i, _i, C.POINTER(_ll)]),
    "enerf_composite_cache_build_workspace_bytes": (C.c_size_t, [_i, _i]),
    "enerf_composite_cache_build": (_i, [C.POINTER(CompositeCacheStruct), _f, _f, _f, _f, _f, _f, C.POINTER(Cascade), _i, C.c_void_p,
                                         C.c_size_t, C.POINTER(Options), _f]),
    "enerf_composite_prep_indexed": (_i, [C.POINTER(CompositePrepArgs), C.c_void_p, _i, _f, _f, _f]),
    "enerf_forward_composite_cached_workspace_bytes": (C.c_size_t, [C.POINTER(CompositeFrameArgs), C.POINTER(CompositeCacheStruct)]),
    "enerf_forward_composite_cached": (_i, [C.POINTER(CompositeFrameArgs), C.POINTER(CompositeCacheStruct), C.c_void_p, _f]),
    "enerf_build_feature_volume_window_at": (_i, [_f, _f, _f] + [_i] * 8 + [C.c_void_p, _i, _i, _f, _f]),
    "enerf_depth_regression_window_at": (_i, [_f, _f] + [_i] * 4 + [C.c_void_p, _i, _i, _i, _f, _f, _f]),
    "enerf_composite_layers_at": (_i, [C.POINTER(CompositeLayersArgs), C.c_void_p, _f]),
    "enerf_layer_boxes": (_i, [_f, _f, _f, _i, _i, _i, C.POINTER(_i), _fl, _f, _f, C.c_void_p, _f]),
    "enerf_forward_composite_moving_workspace_bytes": (C.c_size_t, [C.POINTER(CompositeFrameArgs)]),
    "enerf_forward_composite_moving": (_i, [C.POINTER(CompositeFrameArgs), _f, C.c_void_p, _f]),
    "enerf_forward_composite_cached_moving_workspace_bytes": (C.c_size_t, [C.POINTER(CompositeFrameArgs), C.POINTER(CompositeCacheStruct)]),
    "enerf_forward_composite_cached_moving": (_i, [C.POINTER(CompositeFrameArgs), C.POINTER(CompositeCacheStruct), C.c_void_p, _f,
                                                   C.c_void_p, _f]),
    "enerf_vhull_workspace_bytes": (C.c_size_t, [C.POINTER(VhullArgs)]),
    "enerf_vhull_bounds": (_i, [C.POINTER(VhullArgs), _f]),
}
EXPORTED_SYMBOLS = tuple(_SIGNATURES)


class EnerfError(RuntimeError):
    pass


def _out(out, shape, device, what):
    """``out`` if given — checked to be a contiguous float32 tensor of ``shape`` on ``device`` — else a fresh tensor."""
    if out is None:
        return torch.empty(shape, dtype=torch.float32, device=device)
    if tuple(out.shape) != tuple(shape) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != device:
        raise EnerfError(f"{what}: out must be a contiguous float32 tensor of shape {tuple(shape)} on {device}")
    return out


def _ptr(t: Optional[torch.Tensor]):
    if t is None:
        return None
    if t.dtype != torch.float32 or not t.is_contiguous():
        raise EnerfError(f"expected contiguous float32 tensor, got {t.dtype} contiguous={t.is_contiguous()}")
    return t.data_ptr()


class EnerfLib:
    """Thin typed wrapper over the shared library.  ``path`` is only overridden by tests (CPU-emulated
    twin built from the same kernel sources); the product always loads :data:`LIB_PATH`."""

    def __init__(self, path: str = LIB_PATH):
        if not os.path.exists(path):
            raise EnerfError(f"{path} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                             "(hipcc --offload-arch=gfx950); there is no fallback path")
        self.path = path
        self.dll = C.CDLL(path)
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(self.dll, name)          # raises AttributeError if a symbol is missing
            fn.restype, fn.argtypes = res, args
        v = self.dll.enerf_abi_version()
        if v != ABI_VERSION:
            raise EnerfError(f"ABI version mismatch: library {v}, binding {ABI_VERSION}")

    # -- plumbing --------------------------------------------------------------------------------
    @staticmethod
    def stream_of(t: torch.Tensor):
        return torch.cuda.current_stream(t.device).cuda_stream if t.is_cuda else None

    _tls = threading.local()           # .keep: a list while wgrad_reduce_batch() is open ON THIS THREAD (the C side records per thread too):
                                       # the partial sums must outlive their wrapper calls

    @property
    def _deferred_scratch(self):
        return getattr(self._tls, "keep", None)

    @_deferred_scratch.setter
    def _deferred_scratch(self, value):
        self._tls.keep = value

    def _scratch(self, nbytes: int, device):
        """Per-call scratch from torch's caching allocator (stream-ordered, graph-capture safe)."""
        t = torch.empty((max(int(nbytes), 1),), dtype=torch.uint8, device=device)
        keep = self._deferred_scratch
        if keep is not None:
            keep.append(t)
        return t

    @contextlib.contextmanager
    def wgrad_reduce_batch(self, ref):
        """ABI v11: inside the block the second stage of every enerf_conv_wgrad / enerf_gemm_wgrad call (the reduction of the blocks'
        partial sums into grad_w) is recorded instead of launched, and ONE kernel runs them all on leaving it (on ``ref``'s stream):
        the gradients returned inside the block are complete only after it.  Same arithmetic, same bits."""
        if os.environ.get("ENERF_WGRAD_DEFER", "1") == "0":       # A/B only (tools/gpu_r06_defer_ab.sh): immediate second stages
            yield
            return
        self._check(self.dll.enerf_wgrad_reduce_begin(), "wgrad_reduce_begin")
        self._deferred_scratch = []
        try:
            yield
        finally:
            try:
                self._check(self.dll.enerf_wgrad_reduce_flush(self.stream_of(ref)), "wgrad_reduce_flush")
            finally:
                self._deferred_scratch = None

    def _check(self, rc: int, what: str):
        if rc != 0:
            raise EnerfError(f"{what} failed ({rc}): {self.dll.enerf_last_error().decode()}")

    # -- entry points -----------------------------------------------------------------------------
    def channels_last(self, src, n, C_, P, Cpad=None):
        Cpad = Cpad or C_
        dst = torch.empty((n, P, Cpad), dtype=torch.float32, device=src.device)
        self._check(self.dll.enerf_channels_last(_ptr(src), _ptr(dst), n, C_, P, Cpad, self.stream_of(src)),
                    "channels_last")
        return dst

    def channels_first(self, src, n, C_, P, Cpad=None):
        Cpad = Cpad or C_
        dst = torch.empty((n, C_, P), dtype=torch.float32, device=src.device)
        self._check(self.dll.enerf_channels_first(_ptr(src), _ptr(dst), n, C_, P, Cpad, self.stream_of(src)),
                    "channels_first")
        return dst

    def pack_img_feat_rgb(self, im_feat, src_inps, Hr, Wr):
        n_img, Cf, Hf, Wf = im_feat.shape
        H, W = src_inps.shape[-2:]
        tex = 4 * ((Cf + 3 + 3) // 4)
        out = torch.empty((n_img, Hr, Wr, tex), dtype=torch.float32, device=im_feat.device)
        self._check(self.dll.enerf_pack_img_feat_rgb(_ptr(im_feat), Cf, Hf, Wf, _ptr(src_inps), H, W, Hr, Wr, tex,
                                                     n_img, _ptr(out), self.stream_of(out)), "pack_img_feat_rgb")
        return out

    def feature_net_pack(self, raw: FeatNetRaw, device):
        n = self.dll.enerf_feature_net_packed_floats()
        packed = torch.empty((n,), dtype=torch.float32, device=device)
        self._check(self.dll.enerf_feature_net_pack(C.byref(raw), _ptr(packed), self.stream_of(packed)),
                    "feature_net_pack")
        return packed

    FEAT_ALL, FEAT_TRUNK, FEAT_LEVEL1, FEAT_LEVEL2 = 0, 1, 2, 3

    def feature_net_alloc(self, src_inps, l2_stride=8, workspace=None):
        """Output / workspace tensors of the FeatureNet for ``src_inps`` (n,3,H,W)."""
        n, _, H, W = src_inps.shape
        dev = src_inps.device
        need = self.dll.enerf_feature_net_workspace_bytes(n, H, W)
        if workspace is None or workspace.numel() * 4 < need:
            workspace = torch.empty(((need + 3) // 4,), dtype=torch.float32, device=dev)
        f0 = torch.empty((n, H // 4, W // 4, 32), dtype=torch.float32, device=dev)
        f1 = torch.empty((n, H // 2, W // 2, 16), dtype=torch.float32, device=dev)
        f2 = torch.empty((n, H, W, l2_stride), dtype=torch.float32, device=dev)
        return f0, f1, f2, workspace

    def feature_net_stage(self, packed, src_inps, bufs, stage, l2_stride=8, options=None):
        """One stage (FEAT_TRUNK / FEAT_LEVEL1 / FEAT_LEVEL2, or FEAT_ALL) on the current stream."""
        n, _, H, W = src_inps.shape
        f0, f1, f2, workspace = bufs
        self._check(self.dll.enerf_feature_net_stage(_ptr(packed), _ptr(src_inps), n, H, W, _ptr(f0), _ptr(f1),
                                                     _ptr(f2), l2_stride, _ptr(workspace), workspace.numel() * 4,
                                                     int(stage), _opt(options), self.stream_of(src_inps)),
                    "feature_net_stage")

    def feature_net(self, packed, src_inps, l2_stride=8, workspace=None, options=None):
        """src_inps (n,3,H,W) -> channels-last (n,H/4,W/4,32), (n,H/2,W/2,16), (n,H,W,l2_stride)."""
        n, _, H, W = src_inps.shape
        f0, f1, f2, workspace = self.feature_net_alloc(src_inps, l2_stride, workspace)
        self._check(self.dll.enerf_feature_net(_ptr(packed), _ptr(src_inps), n, H, W, _ptr(f0), _ptr(f1), _ptr(f2),
                                               l2_stride, _ptr(workspace), workspace.numel() * 4, _opt(options),
                                               self.stream_of(src_inps)), "feature_net")
        return f0, f1, f2, workspace

    def pack_texels_cl(self, feat_cl, src_inps, Hr, Wr, out=None):
        n_img, hf, wf, Cf = feat_cl.shape
        if (hf, wf) != (Hr, Wr):
            raise EnerfError("pack_texels_cl: features must already be at the render resolution")
        H, W = src_inps.shape[-2:]
        tex = 4 * ((Cf + 3 + 3) // 4)
        out = _out(out, (n_img, Hr, Wr, tex), feat_cl.device, "pack_texels_cl")
        self._check(self.dll.enerf_pack_texels_cl(_ptr(feat_cl), Cf, _ptr(src_inps), H, W, Hr, Wr, tex, n_img, _ptr(out),
                                                  self.stream_of(out)), "pack_texels_cl")
        return out

    def get_proj_mats(self, src_ixts, src_exts, tar_ixt, tar_ext, src_scale, tar_scale, out=None):
        B, S = src_ixts.shape[:2]
        proj = _out(out, (B, S, 3, 4), src_ixts.device, "get_proj_mats")
        self._check(self.dll.enerf_get_proj_mats(_ptr(src_ixts), _ptr(src_exts), _ptr(tar_ixt), _ptr(tar_ext), B, S,
                                                 float(src_scale), float(tar_scale), _ptr(proj),
                                                 self.stream_of(proj)), "get_proj_mats")
        return proj

    def get_depth_values(self, near_far, prev, B, D, h, w, depth_inv, out=None):
        dev = near_far.device
        dv = _out(None if out is None else out[0], (B, D, h, w), dev, "get_depth_values")
        nf = _out(None if out is None else out[1], (B, 2, h, w), dev, "get_depth_values")
        if prev is None:
            pd = ps = pn = None
            hp = wp = 0
        else:
            pd, ps, pn = prev
            hp, wp = pd.shape[-2:]
        self._check(self.dll.enerf_get_depth_values(_ptr(near_far), _ptr(pd), _ptr(ps), _ptr(pn), B, D, h, w, hp, wp,
                                                    int(depth_inv), _ptr(dv), _ptr(nf), self.stream_of(dv)),
                    "get_depth_values")
        return dv, nf

    def level_prep(self, src_ixts, src_exts, tar_ixt, tar_ext, src_scale, tar_scale, near_far, prev, D, h, w, depth_inv):
        """get_proj_mats + get_depth_values of one level in one launch -> (proj, depth_values, near_far)."""
        B, S = src_ixts.shape[:2]
        dev = src_ixts.device
        proj = torch.empty((B, S, 3, 4), dtype=torch.float32, device=dev)
        dv = torch.empty((B, D, h, w), dtype=torch.float32, device=dev)
        nf = torch.empty((B, 2, h, w), dtype=torch.float32, device=dev)
        if prev is None:
            pd = ps = pn = None
            hp = wp = 0
        else:
            pd, ps, pn = prev
            hp, wp = pd.shape[-2:]
        self._check(self.dll.enerf_level_prep(_ptr(src_ixts), _ptr(src_exts), _ptr(tar_ixt), _ptr(tar_ext), B, S,
                                              float(src_scale), float(tar_scale), _ptr(proj), _ptr(near_far), _ptr(pd),
                                              _ptr(ps), _ptr(pn), D, h, w, hp, wp, int(depth_inv), _ptr(dv), _ptr(nf),
                                              self.stream_of(dv)), "level_prep")
        return proj, dv, nf

    def build_feature_volume(self, feat_cl, proj, dv, Cc, out=None):
        B, S, Hs, Ws = feat_cl.shape[:4]
        _, D, h, w = dv.shape
        vol = _out(out, (B, D, h, w, Cc), dv.device, "build_feature_volume")
        self._check(self.dll.enerf_build_feature_volume(_ptr(feat_cl), _ptr(proj), _ptr(dv), B, S, Cc, Hs, Ws, D, h, w,
                                                        _ptr(vol), self.stream_of(vol)), "build_feature_volume")
        return vol

    def cost_reg_pack(self, raw: CostRegRaw, device):
        n = self.dll.enerf_cost_reg_packed_floats(raw.in_channels, raw.full)
        packed = torch.empty((n,), dtype=torch.float32, device=device)
        self._check(self.dll.enerf_cost_reg_pack(C.byref(raw), _ptr(packed), self.stream_of(packed)), "cost_reg_pack")
        return packed

    def cost_reg(self, packed, in_channels, full, vol, workspace=None, options=None, out=None):
        B, D, h, w, _ = vol.shape
        need = self.dll.enerf_cost_reg_workspace_bytes(int(full), B, D, h, w)
        if workspace is None or workspace.numel() * 4 < need:
            workspace = torch.empty(((need + 3) // 4,), dtype=torch.float32, device=vol.device)
        feat = _out(None if out is None else out[0], (B, D, h, w, 8), vol.device, "cost_reg")
        prob = _out(None if out is None else out[1], (B, D, h, w), vol.device, "cost_reg")
        self._check(self.dll.enerf_cost_reg(_ptr(packed), in_channels, int(full), _ptr(vol), B, D, h, w, _ptr(feat),
                                            _ptr(prob), _ptr(workspace), workspace.numel() * 4, _opt(options),
                                            self.stream_of(vol)), "cost_reg")
        return feat, prob

    def cost_reg_prob(self, packed, in_channels, full, vol, workspace=None, options=None, out=None):
        """prob of ``cost_reg`` alone (``enerf_cost_reg_prob``): the fused heads skip the feature channels."""
        B, D, h, w, _ = vol.shape
        need = self.dll.enerf_cost_reg_workspace_bytes(int(full), B, D, h, w)
        if workspace is None or workspace.numel() * 4 < need:
            workspace = torch.empty(((need + 3) // 4,), dtype=torch.float32, device=vol.device)
        prob = _out(out, (B, D, h, w), vol.device, "cost_reg_prob")
        self._check(self.dll.enerf_cost_reg_prob(_ptr(packed), in_channels, int(full), _ptr(vol), B, D, h, w, _ptr(prob),
                                                 _ptr(workspace), workspace.numel() * 4, _opt(options), self.stream_of(vol)),
                    "cost_reg_prob")
        return prob

    def depth_regression(self, prob, dv, depth_inv, out=None):
        B, D, h, w = prob.shape
        depth = _out(None if out is None else out[0], (B, h, w), prob.device, "depth_regression")
        std = _out(None if out is None else out[1], (B, h, w), prob.device, "depth_regression")
        self._check(self.dll.enerf_depth_regression(_ptr(prob), _ptr(dv), B, D, h, w, int(depth_inv), _ptr(depth),
                                                    _ptr(std), self.stream_of(prob)), "depth_regression")
        return depth, std

    def build_rays(self, rays8, depth, std, near_far, Hr, Wr, depth_inv):
        B, N = rays8.shape[:2]
        h, w = depth.shape[-2:]
        out = torch.empty((B, N, 12), dtype=torch.float32, device=rays8.device)
        self._check(self.dll.enerf_build_rays(_ptr(rays8), _ptr(depth), _ptr(std), _ptr(near_far), B, N, h, w, Hr, Wr,
                                              int(depth_inv), _ptr(out), self.stream_of(out)), "build_rays")
        return out

    def nerf_pack(self, raw: NerfRaw, F: int, viewdir_agg: bool, device):
        n = self.dll.enerf_nerf_packed_floats(F)
        packed = torch.empty((n,), dtype=torch.float32, device=device)
        self._check(self.dll.enerf_nerf_pack(C.byref(raw), F, int(viewdir_agg), _ptr(packed),
                                             self.stream_of(packed)), "nerf_pack")
        return packed

    def render_rays(self, rays12, tex, vol, src_exts, src_ixts, tar_ext, packed, *, n_samples, depth_inv, F,
                    render_scale, white_bkgd=False, maps=None, options=None, max_blocks=0, ray_index=None, ray_count=None,
                    scatter_rgb=False, out=None):
        """``rays12`` (B,N,12) from build_rays — or, with ``maps=(depth, std, near_far)`` of the level, the
        8-float rays (B,N,8): build_rays then runs inside the render kernel.

        ``max_blocks`` > 0 caps the launch at that many persistent blocks.  ``ray_index`` (int32, device) with ``ray_count``
        ((1,) int32, device; B must be 1) renders rays ``ray_index[:ray_count]`` only: depth / weights (and rgb, unless
        ``scatter_rgb``) land compacted in rows ``[0, ray_count)``; with ``scatter_rgb`` rgb goes to row ``ray_index[r]`` (and
        nowhere when ``ray_count`` <= 1).  Rows the kernel does not write keep what ``out=(rgb, depth, weights)`` held."""
        B, N = rays12.shape[:2]
        if (rays12.shape[-1] != 12) != (maps is not None):
            raise EnerfError("render_rays: pass (B,N,12) rays, or (B,N,8) rays together with maps=(depth,std,near_far)")
        if (ray_index is None) != (ray_count is None):
            raise EnerfError("render_rays: pass both ray_index and ray_count or neither")
        S, Hr, Wr = tex.shape[1:4]
        _, D, h, w, _ = vol.shape
        dev = rays12.device
        if out is None:
            rgb = torch.empty((B, N, 3), dtype=torch.float32, device=dev)
            depth = torch.empty((B, N), dtype=torch.float32, device=dev)
            weights = torch.empty((B, N, n_samples), dtype=torch.float32, device=dev)
        else:
            rgb, depth, weights = out
            if (tuple(rgb.shape), tuple(depth.shape), tuple(weights.shape)) != ((B, N, 3), (B, N), (B, N, n_samples)):
                raise EnerfError("render_rays: out=(rgb, depth, weights) must be (B,N,3), (B,N), (B,N,n_samples)")
            for t in out:
                if t.dtype != torch.float32 or not t.is_contiguous() or t.device != dev:
                    raise EnerfError("render_rays: out=(rgb, depth, weights) must be contiguous float32 on the rays' device")
        if ray_index is not None:
            for t in (ray_index, ray_count):
                if t.dtype != torch.int32 or not t.is_contiguous() or t.device != dev:
                    raise EnerfError("render_rays: ray_index / ray_count must be contiguous int32 on the rays' device")
            if ray_index.numel() < N or ray_count.numel() < 1:
                raise EnerfError("render_rays: ray_index needs N entries and ray_count one")
        if maps is None:
            fused = (None, None, None, None, 0, 0)
            r12 = _ptr(rays12)
        else:
            md, ms, mn = maps
            fused = (_ptr(rays12), _ptr(md), _ptr(ms), _ptr(mn), int(md.shape[-2]), int(md.shape[-1]))
            r12 = None
        a = RenderArgs(r12, _ptr(tex), _ptr(vol), _ptr(src_exts), _ptr(src_ixts), _ptr(tar_ext),
                       _ptr(packed), _ptr(rgb), _ptr(depth), _ptr(weights), B, N, S, n_samples, int(depth_inv), Hr,
                       Wr, F, D, h, w, int(white_bkgd), float(render_scale), *fused,
                       None if options is None else C.pointer(options),
                       None if ray_index is None else ray_index.data_ptr(),
                       None if ray_count is None else ray_count.data_ptr(), int(bool(scatter_rgb)), int(max_blocks))
        self._check(self.dll.enerf_render_rays(C.byref(a), self.stream_of(rays12)), "render_rays")
        return rgb, depth, weights

    # -- the composite network (network_composite.py): windows are (x0, y0, ww, wh) in pixels of the grid they are cut from ------
    def build_feature_volume_window(self, feat_cl, proj, dv, Cc, window, out=None):
        """The cost volume of the voxels inside ``window`` of dv's (h, w) grid: (B, D, wh, ww, Cc), the bits of the full volume."""
        B, S, Hs, Ws = feat_cl.shape[:4]
        _, D, h, w = dv.shape
        x0, y0, ww, wh = (int(v) for v in window)
        vol = _out(out, (B, D, max(wh, 0), max(ww, 0), Cc), dv.device, "build_feature_volume_window")
        self._check(self.dll.enerf_build_feature_volume_window(_ptr(feat_cl), _ptr(proj), _ptr(dv), B, S, Cc, Hs, Ws, D, h, w, x0, y0, ww,
                                                               wh, _ptr(vol), self.stream_of(vol)), "build_feature_volume_window")
        return vol

    def depth_regression_window(self, prob, dv, depth_inv, window, out=None):
        """depth_regression of ``prob`` (B, D, wh, ww) zero-padded to dv's (B, D, h, w) grid, without the padded tensor."""
        B, D, h, w = dv.shape
        x0, y0, ww, wh = (int(v) for v in window)
        if tuple(prob.shape) != (B, D, wh, ww):
            raise EnerfError(f"depth_regression_window: prob {tuple(prob.shape)} is not (B, D, wh, ww) = {(B, D, wh, ww)}")
        depth = _out(None if out is None else out[0], (B, h, w), dv.device, "depth_regression_window")
        std = _out(None if out is None else out[1], (B, h, w), dv.device, "depth_regression_window")
        self._check(self.dll.enerf_depth_regression_window(_ptr(prob), _ptr(dv), B, D, h, w, x0, y0, ww, wh, int(depth_inv), _ptr(depth),
                                                           _ptr(std), self.stream_of(dv)), "depth_regression_window")
        return depth, std

    def window_ray_index(self, window, Hr, Wr, device, out=None):
        """(index, count) on the device for render_rays_raw's selection: the window's pixels in the (Hr, Wr) raster, raster order."""
        x0, y0, ww, wh = (int(v) for v in window)
        index, count = out if out is not None else (torch.empty((max(ww * wh, 1),), dtype=torch.int32, device=device),
                                                    torch.empty((1,), dtype=torch.int32, device=device))
        if index.dtype != torch.int32 or count.dtype != torch.int32 or index.numel() < ww * wh or count.numel() < 1:
            raise EnerfError("window_ray_index: out=(index, count) must be int32 with ww*wh entries and one")
        self._check(self.dll.enerf_window_ray_index(x0, y0, ww, wh, int(Hr), int(Wr), index.data_ptr(), count.data_ptr(),
                                                    self.stream_of(index)), "window_ray_index")
        return index, count

    def render_rays_raw(self, rays, tex, vol, src_exts, src_ixts, tar_ext, packed, *, n_samples, depth_inv, F, render_scale, maps=None,
                        max_blocks=0, ray_index=None, ray_count=None, n_out=None, out=None):
        """The render kernel up to the MLP: ``raw`` (B, n, n_samples, 4) = [r, g, b, sigma] and ``z`` (B, n, n_samples), the samples'
        metric depths.  ``rays`` as in :meth:`render_rays`; ``vol`` may be None (the MLP's eight voxel inputs are then zero).
        With ``ray_index`` / ``ray_count`` (B == 1) rows are compacted; ``n_out`` is then the number of rows to allocate."""
        B, N = rays.shape[:2]
        if (rays.shape[-1] != 12) != (maps is not None):
            raise EnerfError("render_rays_raw: pass (B,N,12) rays, or (B,N,8) rays together with maps=(depth,std,near_far)")
        if (ray_index is None) != (ray_count is None):
            raise EnerfError("render_rays_raw: pass both ray_index and ray_count or neither")
        S, Hr, Wr = tex.shape[1:4]
        D, h, w = vol.shape[1:4] if vol is not None else (0, 0, 0)
        dev = rays.device
        n = N if n_out is None else int(n_out)
        if out is None:
            raw = torch.empty((B, n, n_samples, 4), dtype=torch.float32, device=dev)
            z = torch.empty((B, n, n_samples), dtype=torch.float32, device=dev)
        else:
            raw, z = out
            if tuple(raw.shape) != (B, n, n_samples, 4) or tuple(z.shape) != (B, n, n_samples):
                raise EnerfError("render_rays_raw: out=(raw, z) must be (B,n,n_samples,4), (B,n,n_samples)")
        if ray_index is not None:
            for t in (ray_index, ray_count):
                if t.dtype != torch.int32 or not t.is_contiguous() or t.device != dev:
                    raise EnerfError("render_rays_raw: ray_index / ray_count must be contiguous int32 on the rays' device")
            if n > ray_index.numel() or n > N:
                raise EnerfError("render_rays_raw: more output rows than selectable rays")
        elif n != N:
            raise EnerfError("render_rays_raw: n_out needs ray_index")
        a = RenderRawArgs()
        if maps is None:
            a.rays12 = _ptr(rays)
        else:
            md, ms, mn = maps
            a.rays8, a.depth_map, a.std_map, a.nf_map = _ptr(rays), _ptr(md), _ptr(ms), _ptr(mn)
            a.map_h, a.map_w = int(md.shape[-2]), int(md.shape[-1])
        a.tex, a.vol, a.src_exts, a.src_ixts, a.tar_ext = _ptr(tex), _ptr(vol), _ptr(src_exts), _ptr(src_ixts), _ptr(tar_ext)
        a.packed, a.raw, a.z = _ptr(packed), _ptr(raw), _ptr(z)
        a.B, a.N, a.S, a.n_samples, a.depth_inv, a.Hr, a.Wr, a.F = B, N, S, int(n_samples), int(depth_inv), Hr, Wr, int(F)
        a.D, a.h, a.w, a.render_scale, a.max_blocks = D, h, w, float(render_scale), int(max_blocks)
        if ray_index is not None:
            a.ray_index, a.ray_count = ray_index.data_ptr(), ray_count.data_ptr()
        self._check(self.dll.enerf_render_rays_raw(C.byref(a), self.stream_of(rays)), "render_rays_raw")
        return raw, z

    def composite_layers(self, fg, windows, bg, H, W, white_bkgd=False, out=None):
        """parse_layer + raw2outputs_composite: ``fg`` = [(raw (n_l, Ns, 4), z (n_l, Ns)), ...] per foreground layer, the rows being the
        pixels of ``windows[l]`` = (x0, y0, ww, wh) in raster order; ``bg`` = (raw (H*W, Ns, 4), z (H*W, Ns)).  Returns a dict with
        rgb (N, 3), depth (N), weights (N, T), net_output (N, T, 4) and z_vals (N, L*Ns), N = H*W, T = (L+1)*Ns.  The reference's
        ``idx`` (torch.sort's permutation) is not returned: equal depths are ordered by layer, then sample, here, and torch.sort
        promises no order for them."""
        L, (bg_raw, bg_z) = len(fg), bg
        Ns, N, dev = int(bg_z.shape[-1]), H * W, bg_z.device
        if L > MAX_FG_LAYERS or len(windows) != L:
            raise EnerfError(f"composite_layers: {L} foreground layers, {len(windows)} windows (at most {MAX_FG_LAYERS}, one window each)")
        if bg_raw.numel() != N * Ns * 4 or bg_z.numel() != N * Ns:
            raise EnerfError("composite_layers: the background covers the whole (H, W) image")
        a = CompositeLayersArgs(L=L, Ns=Ns, H=int(H), W=int(W), white_bkgd=int(bool(white_bkgd)))
        for l, ((raw, z), win) in enumerate(zip(fg, windows)):
            x0, y0, ww, wh = (int(v) for v in win)
            if raw.numel() != max(ww * wh, 0) * Ns * 4 or z.numel() != max(ww * wh, 0) * Ns:
                raise EnerfError(f"composite_layers: layer {l}: buffers do not hold the window's {ww}x{wh} pixels x {Ns} samples")
            a.fg_raw[l], a.fg_z[l] = _ptr(raw), _ptr(z)
            a.win[l][0], a.win[l][1], a.win[l][2], a.win[l][3] = x0, y0, ww, wh
        T = (L + 1) * Ns
        shapes = {"rgb": (N, 3), "depth": (N,), "weights": (N, T), "net_output": (N, T, 4), "z_vals": (N, L * Ns)}
        res = out if out is not None else {k: torch.empty(sh, dtype=torch.float32, device=dev) for k, sh in shapes.items()}
        for k, sh in shapes.items():
            if tuple(res[k].shape) != sh:
                raise EnerfError(f"composite_layers: out[{k!r}] must be {sh}")
            setattr(a, k, _ptr(res[k]))
        a.bg_raw, a.bg_z = _ptr(bg_raw), _ptr(bg_z)
        self._check(self.dll.enerf_composite_layers(C.byref(a), self.stream_of(bg_z)), "composite_layers")
        return res

    def composite_prep(self, src_ixts, src_exts, tar_ixt, tar_ext, near_far, scales, fg_planes, bg_planes, h, w, depth_inv, rasters,
                       windows, view_idx=None):
        """The composite frame's camera-only preparation in one launch.  ``near_far`` (L+1, 2), the background's row last;
        ``scales`` = [(src_scale, tar_scale)] per level; ``rasters`` = [(Hr, Wr) or None] per level; ``windows[i]`` = the L windows
        (x0, y0, ww, wh) of level i's raster (ignored where the raster is None).  Returns ``(proj, dv, nf, index)``: proj[i]
        (1,S,3,4) per level; dv[c] (1,D_c,h,w), nf[c] (1,2,h,w) per cascade; index[i] = [(index, count)] per window, or None.
        With ``view_idx`` (S) int32 on the device (``enerf_composite_prep_indexed``) ``src_ixts`` / ``src_exts`` are the (V,3,3) /
        (V,4,4) tables of a cache, source camera s is their row ``view_idx[s]``, and the gathered rows are returned too:
        ``(proj, dv, nf, index, (cam_exts (1,S,4,4), cam_ixts (1,S,3,3)))``."""
        dev = src_ixts.device
        S = int(src_ixts.shape[1]) if view_idx is None else int(view_idx.numel())
        L = int(near_far.shape[0]) - 1
        if not 1 <= L <= MAX_FG_LAYERS or len(scales) > MAX_LEVELS:
            raise EnerfError(f"composite_prep: L={L} layers (1..{MAX_FG_LAYERS}), {len(scales)} levels (at most {MAX_LEVELS})")
        a = CompositePrepArgs(L=L, S=S, num_levels=len(scales), fg_planes=int(fg_planes), bg_planes=int(bg_planes), h=int(h), w=int(w),
                              depth_inv=int(depth_inv))
        a.src_ixts, a.src_exts, a.tar_ixt, a.tar_ext, a.near_far = (_ptr(t) for t in (src_ixts, src_exts, tar_ixt, tar_ext, near_far))
        proj, dv, nf, index = [], [], [], []
        for i, (ss, ts) in enumerate(scales):
            a.src_scale[i], a.tar_scale[i] = float(ss), float(ts)
            proj.append(torch.empty((1, S, 3, 4), dtype=torch.float32, device=dev))
            a.proj[i] = proj[-1].data_ptr()
            index.append(None)
            if rasters[i] is None:
                continue
            a.Hr[i], a.Wr[i] = int(rasters[i][0]), int(rasters[i][1])
            index[i] = []
            for l in range(L):
                x0, y0, ww, wh = (int(v) for v in windows[i][l])
                pair = (torch.empty((max(ww * wh, 1),), dtype=torch.int32, device=dev), torch.empty((1,), dtype=torch.int32, device=dev))
                index[i].append(pair)
                a.win[i][l][0], a.win[i][l][1], a.win[i][l][2], a.win[i][l][3] = x0, y0, ww, wh
                a.index[i][l], a.count[i][l] = pair[0].data_ptr(), pair[1].data_ptr()
        for c in range(L + 1):
            D = int(fg_planes) if c < L else int(bg_planes)
            dv.append(torch.empty((1, max(D, 0), max(int(h), 0), max(int(w), 0)), dtype=torch.float32, device=dev))
            nf.append(torch.empty((1, 2, max(int(h), 0), max(int(w), 0)), dtype=torch.float32, device=dev))
            a.dv[c], a.nf[c] = dv[-1].data_ptr(), nf[-1].data_ptr()
        if view_idx is not None:
            if view_idx.dtype != torch.int32 or not view_idx.is_contiguous() or view_idx.device != dev:
                raise EnerfError("composite_prep: view_idx must be a contiguous int32 tensor on the cameras' device")
            cams = (torch.empty((1, S, 4, 4), dtype=torch.float32, device=dev), torch.empty((1, S, 3, 3), dtype=torch.float32, device=dev))
            self._check(self.dll.enerf_composite_prep_indexed(C.byref(a), view_idx.data_ptr(), int(src_exts.shape[0]), _ptr(cams[0]),
                                                              _ptr(cams[1]), self.stream_of(src_ixts)), "composite_prep_indexed")
            return proj, dv, nf, index, cams
        self._check(self.dll.enerf_composite_prep(C.byref(a), self.stream_of(src_ixts)), "composite_prep")
        return proj, dv, nf, index

    def forward_composite_workspace_bytes(self, args: "CompositeFrameArgs") -> int:
        n = self.dll.enerf_forward_composite_workspace_bytes(C.byref(args))
        if n == 0:
            raise EnerfError(f"forward_composite: {self.dll.enerf_last_error().decode()}")
        return n

    def forward_composite(self, args: "CompositeFrameArgs", stream):
        self._check(self.dll.enerf_forward_composite(C.byref(args), stream), "forward_composite")

    # -- the composite network's source-view cache (enerf_amd/composite_cache.py owns the tensors) --------
    def composite_cache_sizes(self, cas: "Cascade", V: int, H: int, W: int):
        """Floats per buffer of an ``enerf_composite_cache_t`` (0 = not needed): fg_feat[0..2], fg_tex[0..2], bg_feat[0..2],
        bg_tex[0..2], exts, ixts."""
        floats = (_ll * COMPOSITE_CACHE_BUFFERS)()
        self._check(self.dll.enerf_composite_cache_sizes(C.byref(cas), V, H, W, floats), "composite_cache_sizes")
        return list(floats)

    def composite_cache_build_workspace(self, H: int, W: int, device):
        """Scratch of ``enerf_composite_cache_build`` for HxW images (it does not depend on V)."""
        nb = self.dll.enerf_composite_cache_build_workspace_bytes(H, W)
        return torch.empty(((nb + 3) // 4,), dtype=torch.float32, device=device)

    def composite_cache_build(self, cache: "CompositeCacheStruct", src_inps, bg_src_inps, exts, ixts, packed, packed_bg, cas: "Cascade",
                              chunk=0, options=None, workspace=None):
        ws = workspace if workspace is not None else self.composite_cache_build_workspace(cache.H, cache.W, src_inps.device)
        self._check(self.dll.enerf_composite_cache_build(C.byref(cache), _ptr(src_inps), _ptr(bg_src_inps), _ptr(exts), _ptr(ixts),
                                                         _ptr(packed), _ptr(packed_bg), C.byref(cas), int(chunk), ws.data_ptr(),
                                                         ws.numel() * 4, _opt(options), self.stream_of(src_inps)), "composite_cache_build")

    def forward_composite_cached_workspace_bytes(self, args: "CompositeFrameArgs", cache: "CompositeCacheStruct") -> int:
        n = self.dll.enerf_forward_composite_cached_workspace_bytes(C.byref(args), C.byref(cache))
        if n == 0:
            raise EnerfError(f"forward_composite_cached: {self.dll.enerf_last_error().decode()}")
        return n

    def forward_composite_cached(self, args: "CompositeFrameArgs", cache: "CompositeCacheStruct", view_idx_ptr, stream):
        self._check(self.dll.enerf_forward_composite_cached(C.byref(args), C.byref(cache), view_idx_ptr, stream), "forward_composite_cached")

    # -- the composite network with boxes that move: sizes on the host, positions on the device (include/enerf_hip.h) ----------
    @staticmethod
    def _corner(xy, n, what):
        if not torch.is_tensor(xy) or xy.dtype != torch.int32 or not xy.is_contiguous() or xy.numel() != n:
            raise EnerfError(f"{what}: the corner(s) must be a contiguous int32 device tensor of {n} values")
        return xy

    def build_feature_volume_window_at(self, feat_cl, proj, dv, Cc, xy, size, out=None):
        """:meth:`build_feature_volume_window` with the window's corner ``xy`` = (x0, y0), two int32 on the device, and its extent
        ``size`` = (ww, wh) on the host.  The corner must lie inside the grid (0 <= x0 <= w - ww, 0 <= y0 <= h - wh)."""
        B, S, Hs, Ws = feat_cl.shape[:4]
        _, D, h, w = dv.shape
        ww, wh = (int(v) for v in size)
        self._corner(xy, 2, "build_feature_volume_window_at")
        vol = _out(out, (B, D, max(wh, 0), max(ww, 0), Cc), dv.device, "build_feature_volume_window_at")
        self._check(self.dll.enerf_build_feature_volume_window_at(_ptr(feat_cl), _ptr(proj), _ptr(dv), B, S, Cc, Hs, Ws, D, h, w,
                                                                  xy.data_ptr(), ww, wh, _ptr(vol), self.stream_of(vol)),
                    "build_feature_volume_window_at")
        return vol

    def depth_regression_window_at(self, prob, dv, depth_inv, xy, size, out=None):
        """:meth:`depth_regression_window` with the corner ``xy`` (two int32) on the device and ``size`` = (ww, wh) on the host."""
        B, D, h, w = dv.shape
        ww, wh = (int(v) for v in size)
        self._corner(xy, 2, "depth_regression_window_at")
        if tuple(prob.shape) != (B, D, wh, ww):
            raise EnerfError(f"depth_regression_window_at: prob {tuple(prob.shape)} is not (B, D, wh, ww) = {(B, D, wh, ww)}")
        depth = _out(None if out is None else out[0], (B, h, w), dv.device, "depth_regression_window_at")
        std = _out(None if out is None else out[1], (B, h, w), dv.device, "depth_regression_window_at")
        self._check(self.dll.enerf_depth_regression_window_at(_ptr(prob), _ptr(dv), B, D, h, w, xy.data_ptr(), ww, wh, int(depth_inv),
                                                              _ptr(depth), _ptr(std), self.stream_of(dv)), "depth_regression_window_at")
        return depth, std

    def composite_layers_at(self, fg, win_xy, sizes, bg, H, W, white_bkgd=False):
        """:meth:`composite_layers` with the L windows' corners ``win_xy`` (L,2) int32 on the device and their extents ``sizes`` =
        [(ww, wh)] on the host."""
        L, (bg_raw, bg_z) = len(fg), bg
        Ns, N, dev = int(bg_z.shape[-1]), H * W, bg_z.device
        if L > MAX_FG_LAYERS or len(sizes) != L:
            raise EnerfError(f"composite_layers_at: {L} foreground layers, {len(sizes)} sizes (at most {MAX_FG_LAYERS}, one size each)")
        self._corner(win_xy, 2 * L, "composite_layers_at")
        if bg_raw.numel() != N * Ns * 4 or bg_z.numel() != N * Ns:
            raise EnerfError("composite_layers_at: the background covers the whole (H, W) image")
        a = CompositeLayersArgs(L=L, Ns=Ns, H=int(H), W=int(W), white_bkgd=int(bool(white_bkgd)))
        for l, ((raw, z), (ww, wh)) in enumerate(zip(fg, sizes)):
            if raw.numel() != max(ww * wh, 0) * Ns * 4 or z.numel() != max(ww * wh, 0) * Ns:
                raise EnerfError(f"composite_layers_at: layer {l}: buffers do not hold the window's {ww}x{wh} pixels x {Ns} samples")
            a.fg_raw[l], a.fg_z[l] = _ptr(raw), _ptr(z)
            a.win[l][2], a.win[l][3] = int(ww), int(wh)
        T = (L + 1) * Ns
        shapes = {"rgb": (N, 3), "depth": (N,), "weights": (N, T), "net_output": (N, T, 4), "z_vals": (N, L * Ns)}
        res = {k: torch.empty(sh, dtype=torch.float32, device=dev) for k, sh in shapes.items()}
        for k in shapes:
            setattr(a, k, _ptr(res[k]))
        a.bg_raw, a.bg_z = _ptr(bg_raw), _ptr(bg_z)
        self._check(self.dll.enerf_composite_layers_at(C.byref(a), win_xy.data_ptr(), self.stream_of(bg_z)), "composite_layers_at")
        return res

    def layer_boxes(self, bounds, tar_ext, tar_ixt, H, W, sizes, near_min=0.0, out=None):
        """The foreground layers' box positions for a target camera, on the device (``enerf_layer_boxes``; read_tar of
        enerf_outdoor/enerf.py:156-164 with the rectangle of the rounded corners in place of cv2's raster, which it contains):
        ``bounds`` (L,2,3) world min / max corner per layer, ``tar_ext`` (1,4,4), ``tar_ixt`` (1,3,3), ``sizes`` = [(w, h)] per
        layer on the host.  Returns ``(xy (L,2) float32, near_far (L+1,2), flags (L) int32)``: ``xy`` is what ``batch['bbox_xy']``
        takes; rows 0..L-1 of ``near_far`` = (max(min z, near_min), max z), the background's row is left as it is (``out`` =
        (xy, near_far, flags) to fill existing tensors, e.g. a near_far whose last row the caller has set).  flags: bit 1 = the
        projected rectangle is larger than the size, bit 2 = a corner is behind the camera (xy = (0, 0)), bit 3 = it misses the
        image.  Nothing is read on the host."""
        L, dev = int(bounds.shape[0]), bounds.device
        sizes = [(int(w), int(h)) for w, h in sizes]
        if tuple(bounds.shape) != (L, 2, 3) or tar_ext.numel() != 16 or tar_ixt.numel() != 9 or len(sizes) != L:
            raise EnerfError(f"layer_boxes: bounds (L,2,3), tar_ext (1,4,4), tar_ixt (1,3,3) and L sizes, got {tuple(bounds.shape)} / "
                             f"{tuple(tar_ext.shape)} / {tuple(tar_ixt.shape)} / {len(sizes)}")
        for t in (bounds, tar_ext, tar_ixt):
            if t.dtype != torch.float32 or not t.is_contiguous() or t.device != dev:
                raise EnerfError("layer_boxes: bounds, tar_ext and tar_ixt must be contiguous float32 tensors on one device")
        if out is None:
            out = (torch.empty((L, 2), dtype=torch.float32, device=dev), torch.zeros((L + 1, 2), dtype=torch.float32, device=dev),
                   torch.empty((L,), dtype=torch.int32, device=dev))
        xy, near_far, flags = out
        if xy.dtype != torch.float32 or xy.numel() != 2 * L or near_far.dtype != torch.float32 or near_far.numel() != 2 * (L + 1) or \
                flags.dtype != torch.int32 or flags.numel() != L or not (xy.is_contiguous() and near_far.is_contiguous()):
            raise EnerfError("layer_boxes: out = (xy (L,2) float32, near_far (L+1,2) float32, flags (L) int32), contiguous")
        host = (_i * (2 * max(L, 1)))(*[v for s_ in sizes for v in s_])
        self._check(self.dll.enerf_layer_boxes(_ptr(bounds), _ptr(tar_ext), _ptr(tar_ixt), L, int(H), int(W), host, float(near_min),
                                               _ptr(xy), _ptr(near_far), flags.data_ptr(), self.stream_of(bounds)), "layer_boxes")
        return xy, near_far, flags

    def forward_composite_moving_workspace_bytes(self, args: "CompositeFrameArgs", cache: "CompositeCacheStruct" = None) -> int:
        n = (self.dll.enerf_forward_composite_moving_workspace_bytes(C.byref(args)) if cache is None else
             self.dll.enerf_forward_composite_cached_moving_workspace_bytes(C.byref(args), C.byref(cache)))
        if n == 0:
            raise EnerfError(f"forward_composite_moving: {self.dll.enerf_last_error().decode()}")
        return n

    def forward_composite_moving(self, args: "CompositeFrameArgs", bbox_xy_ptr, flags_ptr, stream, cache=None, view_idx_ptr=None):
        if cache is None:
            self._check(self.dll.enerf_forward_composite_moving(C.byref(args), bbox_xy_ptr, flags_ptr, stream), "forward_composite_moving")
        else:
            self._check(self.dll.enerf_forward_composite_cached_moving(C.byref(args), C.byref(cache), view_idx_ptr, bbox_xy_ptr, flags_ptr,
                                                                       stream), "forward_composite_cached_moving")

    # -- backward kernels (training path; wrapped by enerf_amd/autograd.py) -----------------------------
    def build_feature_volume_bwd(self, feat_cl, proj, dv, grad_vol):
        B, S, Hs, Ws, Cc = feat_cl.shape
        _, D, h, w = dv.shape
        gfeat = torch.empty_like(feat_cl)
        gdv = torch.empty_like(dv)
        self._check(self.dll.enerf_build_feature_volume_bwd(_ptr(feat_cl), _ptr(proj), _ptr(dv), _ptr(grad_vol), B, S, Cc, Hs, Ws,
                                                            D, h, w, _ptr(gfeat), _ptr(gdv), self.stream_of(dv)),
                    "build_feature_volume_bwd")
        return gfeat, gdv

    def depth_regression_bwd(self, prob, dv, g_depth, g_std, depth_inv):
        B, D, h, w = prob.shape
        gp, gdv = torch.empty_like(prob), torch.empty_like(dv)
        self._check(self.dll.enerf_depth_regression_bwd(_ptr(prob), _ptr(dv), _ptr(g_depth), _ptr(g_std), B, D, h, w,
                                                        int(depth_inv), _ptr(gp), _ptr(gdv), self.stream_of(prob)),
                    "depth_regression_bwd")
        return gp, gdv

    # -- backward kernels of the composite network (windows as in the forward methods) --
    def build_feature_volume_window_bwd(self, feat_cl, proj, dv, grad_vol, window):
        """Backward of :meth:`build_feature_volume_window`: ``grad_vol`` (B, D, wh, ww, C) -> (grad_feat like ``feat_cl``, grad_dv
        like ``dv``; exactly 0 outside the window)."""
        B, S, Hs, Ws, Cc = feat_cl.shape
        _, D, h, w = dv.shape
        x0, y0, ww, wh = (int(v) for v in window)
        if tuple(grad_vol.shape) != (B, D, wh, ww, Cc) or not grad_vol.is_contiguous():
            raise EnerfError(f"build_feature_volume_window_bwd: grad_vol {tuple(grad_vol.shape)} is not a contiguous {(B, D, wh, ww, Cc)}")
        gfeat, gdv = torch.empty_like(feat_cl), torch.empty_like(dv)
        self._check(self.dll.enerf_build_feature_volume_window_bwd(_ptr(feat_cl), _ptr(proj), _ptr(dv), _ptr(grad_vol), B, S, Cc, Hs, Ws,
                                                                   D, h, w, x0, y0, ww, wh, _ptr(gfeat), _ptr(gdv), self.stream_of(dv)),
                    "build_feature_volume_window_bwd")
        return gfeat, gdv

    def depth_regression_window_bwd(self, prob, dv, g_depth, g_std, depth_inv, window):
        """Backward of :meth:`depth_regression_window`: ``g_depth`` / ``g_std`` (B, h, w) over the full image -> (grad_prob like
        ``prob``, grad_dv like ``dv``)."""
        B, D, h, w = dv.shape
        x0, y0, ww, wh = (int(v) for v in window)
        if tuple(prob.shape) != (B, D, wh, ww) or tuple(g_depth.shape) != (B, h, w) or tuple(g_std.shape) != (B, h, w):
            raise EnerfError(f"depth_regression_window_bwd: prob {tuple(prob.shape)} is not {(B, D, wh, ww)}, or g_depth / g_std "
                             f"{tuple(g_depth.shape)} / {tuple(g_std.shape)} not {(B, h, w)}")
        gp, gdv = torch.empty_like(prob), torch.empty_like(dv)
        self._check(self.dll.enerf_depth_regression_window_bwd(_ptr(prob), _ptr(dv), _ptr(g_depth), _ptr(g_std), B, D, h, w, x0, y0, ww,
                                                               wh, int(depth_inv), _ptr(gp), _ptr(gdv), self.stream_of(dv)),
                    "depth_regression_window_bwd")
        return gp, gdv

    def composite_layers_bwd(self, fg, windows, bg, H, W, g_rgb, g_depth, g_weights, white_bkgd=False, out=None):
        """Backward of :meth:`composite_layers` (same ``fg``, ``windows``, ``bg``): upstream ``g_rgb`` (N, 3), ``g_depth`` (N),
        ``g_weights`` (N, T), each optional (None = zeros).  Returns ``([grad_raw per layer], grad_bg_raw)`` shaped like the raw
        inputs; the depths receive no gradient.  ``out`` = the same pair, preallocated."""
        L, (bg_raw, bg_z) = len(fg), bg
        Ns, N = int(bg_z.shape[-1]), H * W
        if L > MAX_FG_LAYERS or len(windows) != L:
            raise EnerfError(f"composite_layers_bwd: {L} foreground layers, {len(windows)} windows (at most {MAX_FG_LAYERS}, one window each)")
        if bg_raw.numel() != N * Ns * 4 or bg_z.numel() != N * Ns:
            raise EnerfError("composite_layers_bwd: the background covers the whole (H, W) image")
        T = (L + 1) * Ns
        for name, t, n in (("g_rgb", g_rgb, N * 3), ("g_depth", g_depth, N), ("g_weights", g_weights, N * T)):
            if t is not None and (t.numel() != n or not t.is_contiguous()):
                raise EnerfError(f"composite_layers_bwd: {name} must be contiguous with {n} elements")
        g_fg, g_bg = out if out is not None else ([torch.empty_like(raw) for raw, _ in fg], torch.empty_like(bg_raw))
        a = CompositeLayersBwdArgs()
        a.fwd.L, a.fwd.Ns, a.fwd.H, a.fwd.W, a.fwd.white_bkgd = L, Ns, int(H), int(W), int(bool(white_bkgd))
        for l, ((raw, z), win) in enumerate(zip(fg, windows)):
            x0, y0, ww, wh = (int(v) for v in win)
            if raw.numel() != max(ww * wh, 0) * Ns * 4 or z.numel() != max(ww * wh, 0) * Ns or g_fg[l].numel() != raw.numel():
                raise EnerfError(f"composite_layers_bwd: layer {l}: buffers do not hold the window's {ww}x{wh} pixels x {Ns} samples")
            a.fwd.fg_raw[l], a.fwd.fg_z[l], a.grad_fg_raw[l] = _ptr(raw), _ptr(z), _ptr(g_fg[l])
            a.fwd.win[l][0], a.fwd.win[l][1], a.fwd.win[l][2], a.fwd.win[l][3] = x0, y0, ww, wh
        if g_bg.numel() != bg_raw.numel():
            raise EnerfError("composite_layers_bwd: out's background gradient must be shaped like bg_raw")
        a.fwd.bg_raw, a.fwd.bg_z, a.grad_bg_raw = _ptr(bg_raw), _ptr(bg_z), _ptr(g_bg)
        a.grad_rgb, a.grad_depth, a.grad_weights = _ptr(g_rgb), _ptr(g_depth), _ptr(g_weights)
        self._check(self.dll.enerf_composite_layers_bwd(C.byref(a), self.stream_of(bg_z)), "composite_layers_bwd")
        return g_fg, g_bg

    # training-mode 3-D conv layers / BatchNorm pieces (train.hip); kind: 0 stride 1, 1 stride 2, 2 transposed stride 2
    def conv3d_layer_pack(self, w, cin, cout, kind):
        packed = torch.empty((self.dll.enerf_conv3d_layer_packed_floats(cin, cout, kind),), dtype=torch.float32, device=w.device)
        self._check(self.dll.enerf_conv3d_layer_pack(_ptr(w), cin, cout, kind, _ptr(packed), self.stream_of(w)), "conv3d_layer_pack")
        return packed

    def conv3d_layer(self, packed, cin, cout, kind, x_cl, residual=None, options=None):
        """x_cl (B,D,h,w,cin) channels-last -> (B,D',h',w',cout); D' = D (kind 0), ceil(D/2) (kind 1), 2D (kind 2)."""
        B, D, h, w, _ = x_cl.shape
        if kind == 1:
            Do, Ho, Wo = (D - 1) // 2 + 1, (h - 1) // 2 + 1, (w - 1) // 2 + 1
        elif kind == 2:
            Do, Ho, Wo = 2 * D, 2 * h, 2 * w
        else:
            Do, Ho, Wo = D, h, w
        out = torch.empty((B, Do, Ho, Wo, cout), dtype=torch.float32, device=x_cl.device)
        self._check(self.dll.enerf_conv3d_layer(_ptr(packed), cin, cout, kind, _ptr(x_cl), _ptr(residual), _ptr(out), B, D, h, w,
                                                _opt(options), self.stream_of(x_cl)), "conv3d_layer")
        return out

    # training-mode FeatureNet convolutions (train.hip: enerf_conv2d_layer): weights (cout,cin,k,k), padding (k-1)/2
    def conv2d_layer_pack(self, w, bias, cin, cout, k):
        packed = torch.empty((self.dll.enerf_conv2d_layer_packed_floats(cin, cout, k),), dtype=torch.float32, device=w.device)
        self._check(self.dll.enerf_conv2d_layer_pack(_ptr(w), _ptr(bias), cin, cout, k, _ptr(packed), self.stream_of(w)), "conv2d_layer_pack")
        return packed

    def conv2d_layer(self, packed, cin, cout, k, stride, x, up=None):
        """x channels-last (N,H,W,cin) — for cin = 3 the NCHW image batch (N,3,H,W) — -> channels-last (N,Ho,Wo,cout);
        ``up`` (N,Ho/2,Wo/2,cout) is upsampled 2x (bilinear, align_corners) and added."""
        if cin == 3:
            N, _, H, W = x.shape
        else:
            N, H, W, _ = x.shape
        P = (k - 1) // 2
        Ho, Wo = (H + 2 * P - k) // stride + 1, (W + 2 * P - k) // stride + 1
        out = torch.empty((N, Ho, Wo, cout), dtype=torch.float32, device=x.device)
        self._check(self.dll.enerf_conv2d_layer(_ptr(packed), cin, cout, k, stride, _ptr(x), _ptr(up), _ptr(out), N, H, W,
                                                self.stream_of(x)), "conv2d_layer")
        return out

    def channel_sums(self, a, b, z_mask=None, mask_scale=None, mask_shift=None):
        """(sum_p a*m, sum_p a*m*b) per channel in fp64; tensors channels-last (..., C)."""
        Cc = a.shape[-1]
        sums = torch.empty((2, Cc), dtype=torch.float64, device=a.device)
        n = a.numel() // Cc
        nb = self.dll.enerf_channel_sums_workspace_bytes(n, Cc)
        ws = self._scratch(nb, a.device)
        self._check(self.dll.enerf_channel_sums_ws(_ptr(a), _ptr(b), _ptr(z_mask), _ptr(mask_scale), _ptr(mask_shift),
                                                   n, Cc, sums.data_ptr(), ws.data_ptr(), nb, self.stream_of(a)), "channel_sums")
        return sums[0], sums[1]

    def up2_adjoint(self, g_fine, add=None):
        """Adjoint of the 2x align-corners bilinear upsampling on a channels-last gradient (N,2h,2w,C) -> (N,h,w,C) (+ add)."""
        N, Hf, Wf, Cc = g_fine.shape
        out = torch.empty((N, Hf // 2, Wf // 2, Cc), dtype=torch.float32, device=g_fine.device)
        self._check(self.dll.enerf_up2_adjoint(_ptr(g_fine), _ptr(add), N, Hf // 2, Wf // 2, Cc, _ptr(out), self.stream_of(g_fine)),
                    "up2_adjoint")
        return out

    def channel_sums_raw(self, a, b, z_mask=None, mask_scale=None, mask_shift=None):
        """channel_sums as ONE (2, C) fp64 tensor [sum a*m ; sum a*m*b] (what the all-reduce and the coefficient kernels take)."""
        Cc = a.shape[-1]
        sums = torch.empty((2, Cc), dtype=torch.float64, device=a.device)
        n = a.numel() // Cc
        nb = self.dll.enerf_channel_sums_workspace_bytes(n, Cc)
        ws = self._scratch(nb, a.device)
        self._check(self.dll.enerf_channel_sums_ws(_ptr(a), _ptr(b), _ptr(z_mask), _ptr(mask_scale), _ptr(mask_shift),
                                                   n, Cc, sums.data_ptr(), ws.data_ptr(), nb, self.stream_of(a)), "channel_sums")
        return sums

    def bn_train_coeffs(self, sums, count, bn):
        """(2,C) fp64 sums + position count (python number, or a 1-element fp64 device tensor) + the BatchNorm module ->
        mean_invstd (2,C) fp64, scale_shift (2,C) fp32; updates the module's running statistics in place."""
        Cc = sums.shape[1]
        mi = torch.empty((2, Cc), dtype=torch.float64, device=sums.device)
        ss = torch.empty((2, Cc), dtype=torch.float32, device=sums.device)
        track = bn.track_running_stats and bn.running_mean is not None      # (num_batches_tracked += 1 happens in the kernel)
        cd, ch = (count.data_ptr(), 0.0) if torch.is_tensor(count) else (None, float(count))
        self._check(self.dll.enerf_bn_train_coeffs(sums.data_ptr(), cd, ch, _ptr(bn.weight.detach()), _ptr(bn.bias.detach()), float(bn.eps),
                                                   -1.0 if bn.momentum is None else float(bn.momentum),
                                                   _ptr(bn.running_mean) if track else None, _ptr(bn.running_var) if track else None,
                                                   bn.num_batches_tracked.data_ptr() if track else None, 1, Cc, mi.data_ptr(), _ptr(ss),
                                                   self.stream_of(sums)), "bn_train_coeffs")
        return mi, ss

    def bn_stats_fit(self, z) -> bool:
        """the channel widths enerf_channel_sums / enerf_bn_train_stats handle (C in 4..64, C/4 dividing 256)"""
        Cc = z.shape[-1]
        return 4 <= Cc <= 64 and Cc % 4 == 0 and 256 % (Cc // 4) == 0

    def bn_train_stats(self, z, bn):
        """ABI v8: batch statistics of z (..., C) AND the forward coefficients of the BatchNorm module in two launches (no
        SyncBatchNorm): -> mean_invstd (2,C) fp64, scale_shift (2,C) fp32; updates the running statistics in place."""
        Cc = z.shape[-1]
        n = z.numel() // Cc
        nb = self.dll.enerf_channel_sums_workspace_bytes(n, Cc)
        ws = self._scratch(nb, z.device)
        mi = torch.empty((2, Cc), dtype=torch.float64, device=z.device)
        ss = torch.empty((2, Cc), dtype=torch.float32, device=z.device)
        track = bn.track_running_stats and bn.running_mean is not None
        self._check(self.dll.enerf_bn_train_stats(_ptr(z), n, Cc, ws.data_ptr(), nb, _ptr(bn.weight.detach()), _ptr(bn.bias.detach()),
                                                  float(bn.eps), -1.0 if bn.momentum is None else float(bn.momentum),
                                                  _ptr(bn.running_mean) if track else None, _ptr(bn.running_var) if track else None,
                                                  bn.num_batches_tracked.data_ptr() if track else None, 1, None, mi.data_ptr(), _ptr(ss),
                                                  self.stream_of(z)), "bn_train_stats")
        return mi, ss, n

    def bn_train_bwd_stats(self, g, z, mean_invstd, scale, z_mask=None, mask_scale=None, mask_shift=None):
        """ABI v8: sums of [g*m, g*m*z] AND the backward coefficients in two launches -> dgamma_dbeta (2,C), k2k3 (2,C)."""
        Cc = z.shape[-1]
        n = z.numel() // Cc
        nb = self.dll.enerf_channel_sums_workspace_bytes(n, Cc)
        ws = self._scratch(nb, z.device)
        dgb = torch.empty((2, Cc), dtype=torch.float32, device=z.device)
        k23 = torch.empty((2, Cc), dtype=torch.float32, device=z.device)
        self._check(self.dll.enerf_bn_train_bwd_stats(_ptr(g), _ptr(z), _ptr(z_mask), _ptr(mask_scale), _ptr(mask_shift), n, Cc, ws.data_ptr(), nb,
                                                      mean_invstd.data_ptr(), _ptr(scale), _ptr(dgb), _ptr(k23), self.stream_of(z)),
                    "bn_train_bwd_stats")
        return dgb, k23

    def bn_train_apply(self, z, bn, residual=None, relu=False):
        """ABI v11: training-mode BatchNorm of z (..., C) (+ ReLU) (+ residual) in two launches for small / mid layers, three otherwise
        (enerf_bn_train_apply) -> (out, mean_invstd (2,C) fp64, scale_shift (2,C) fp32, positions); updates the running statistics."""
        Cc = z.shape[-1]
        n = z.numel() // Cc
        nb = self.dll.enerf_channel_sums_workspace_bytes(n, Cc)
        ws = self._scratch(nb, z.device)
        mi = torch.empty((2, Cc), dtype=torch.float64, device=z.device)
        ss = torch.empty((2, Cc), dtype=torch.float32, device=z.device)
        out = torch.empty_like(z)
        track = bn.track_running_stats and bn.running_mean is not None
        self._check(self.dll.enerf_bn_train_apply(_ptr(z), n, Cc, ws.data_ptr(), nb, _ptr(bn.weight.detach()), _ptr(bn.bias.detach()),
                                                  float(bn.eps), -1.0 if bn.momentum is None else float(bn.momentum),
                                                  _ptr(bn.running_mean) if track else None, _ptr(bn.running_var) if track else None,
                                                  bn.num_batches_tracked.data_ptr() if track else None, 1, mi.data_ptr(), _ptr(ss),
                                                  _ptr(residual), int(relu), _ptr(out), self.stream_of(z)), "bn_train_apply")
        return out, mi, ss, n

    def bn_train_bwd_apply(self, g, z, mean_invstd, scale_shift, relu):
        """ABI v11: (grad_z, dgamma_dbeta (2,C)) of the BatchNorm (+ ReLU) whose forward was bn_train_apply (enerf_bn_train_bwd_apply)."""
        Cc = z.shape[-1]
        n = z.numel() // Cc
        nb = self.dll.enerf_channel_sums_workspace_bytes(n, Cc) + 2 * Cc * 4
        ws = self._scratch(nb, z.device)
        dgb = torch.empty((2, Cc), dtype=torch.float32, device=z.device)
        dz = torch.empty_like(z)
        self._check(self.dll.enerf_bn_train_bwd_apply(_ptr(g), _ptr(z), int(relu), n, Cc, ws.data_ptr(), nb, mean_invstd.data_ptr(),
                                                      _ptr(scale_shift), _ptr(dgb), _ptr(dz), self.stream_of(z)), "bn_train_bwd_apply")
        return dz, dgb

    def bn_train_bwd_coeffs(self, local, glob, count, mean_invstd, scale):
        Cc = local.shape[1]
        dgb = torch.empty((2, Cc), dtype=torch.float32, device=local.device)
        k23 = torch.empty((2, Cc), dtype=torch.float32, device=local.device)
        cd, ch = (count.data_ptr(), 0.0) if torch.is_tensor(count) else (None, float(count))
        self._check(self.dll.enerf_bn_train_bwd_coeffs(local.data_ptr(), glob.data_ptr(), cd, ch, mean_invstd.data_ptr(), _ptr(scale), Cc,
                                                       _ptr(dgb), _ptr(k23), self.stream_of(local)), "bn_train_bwd_coeffs")
        return dgb, k23

    def channel_affine(self, a, p, r, b=None, q=None, z_mask=None, mask_scale=None, mask_shift=None, residual=None, relu=False):
        Cc = a.shape[-1]
        out = torch.empty_like(a)
        self._check(self.dll.enerf_channel_affine(_ptr(a), _ptr(b), _ptr(p), _ptr(q), _ptr(r), _ptr(z_mask), _ptr(mask_scale),
                                                  _ptr(mask_shift), _ptr(residual), int(relu), a.numel() // Cc, Cc, _ptr(out),
                                                  self.stream_of(a)), "channel_affine")
        return out

    def gemm_wgrad(self, a, b, Ca=None, Cb=None, bias=False):
        """grad_w (Ca,Cb) = sum over rows p of a[p,:Ca]^T b[p,:Cb]; a, b 2-D row-major (possibly column slices: a view whose
        rows are wider than Ca is passed by its base pointer + row stride).  bias=True -> (grad_w, grad_bias (Ca) = column
        sums of a) from the same pass."""
        P = a.shape[0]
        Ca, Cb = Ca or a.shape[1], Cb or b.shape[1]
        if a.stride(1) != 1 or b.stride(1) != 1:
            raise EnerfError("gemm_wgrad: rows must be contiguous")
        gw = torch.empty((Ca, Cb), dtype=torch.float32, device=a.device)
        gb = torch.empty((Ca,), dtype=torch.float32, device=a.device) if bias else None
        ws = self._scratch(self.dll.enerf_gemm_wgrad_workspace_bytes(P, Ca, Cb, int(bias)), a.device)
        self._check(self.dll.enerf_gemm_wgrad(a.data_ptr(), a.stride(0), Ca, b.data_ptr(), b.stride(0), Cb, P, _ptr(gw),
                                              _ptr(gb), ws.data_ptr(), ws.numel(), self.stream_of(a)), "gemm_wgrad")
        return (gw, gb) if bias else gw

    SELFTEST_NAMES = ("xor16", "xor32", "group_sum4", "group_max4", "row_sum16", "add_xor8", "group_bcast<2>", "group_bcast<4>",
                      "group_bcast<8>", "glds16 + raw barrier", "raw buffer loads", "mfma 16x16x4 layout", "mfma 4x4x1 broadcast-A",
                      "mfma 4x4x1", "relu1 (med3)", "mul24", "lds / global fp32 atomics", "rcp / sqrt / exp", "wave_sync", "xcd_contiguous")

    def selftest_primitives(self, device, blocks: int = 24):
        """{check name: lanes that disagree with the memory-only specification} (enerf_selftest_primitives): all zero on a sound build."""
        n = self.dll.enerf_selftest_checks()
        assert n == len(self.SELFTEST_NAMES)
        g = torch.Generator().manual_seed(5)
        table = torch.randn(4096, generator=g).to(device)
        scratch = torch.empty(blocks * 16, dtype=torch.float32, device=device)
        bad = torch.empty(n, dtype=torch.int32, device=device)
        self._check(self.dll.enerf_selftest_primitives(_ptr(table), table.numel(), _ptr(scratch), blocks, bad.data_ptr(),
                                                       self.stream_of(table)), "selftest_primitives")
        return dict(zip(self.SELFTEST_NAMES, (int(v) for v in bad.cpu())))

    def gemm_wgrad_group(self, members):
        """Several ``gemm_wgrad`` calls as TWO launches (enerf_gemm_wgrad_group; every gradient bit-identical to its single call).
        ``members``: dicts with ``a``, ``b`` (2-D row-major, possibly column slices), optional ``Cb`` (leading columns of b used),
        ``bias`` (also the column sums of a) and ``into = (matrix (Ca, W), first column)`` — the gradient is a column block of a
        wider weight matrix and is written in place.  Returns one (grad_w or the ``into`` matrix, grad_bias or None) per member."""
        n = len(members)
        descs, out = (GemmWgradDesc * n)(), []
        for d, m in zip(descs, members):
            if m.get("partials") is not None:                  # first stage done elsewhere (nerf_mlp_bwd(partials=True)): reduce only
                part, (mat, c0) = m["partials"], m["into"]
                Ca, Cb = m["Ca"], m["Cb"]
                if part.shape[1] * 16 * 16 < ((Ca + 15) // 16) * ((Cb + 15) // 16) * 256 or not part.is_contiguous() or not mat.is_contiguous():
                    raise EnerfError("gemm_wgrad_group: partial rows do not hold the member's tiles")
                d.Ca, d.Cb, d.grad_w, d.ldw = Ca, Cb, mat.data_ptr() + 4 * c0, mat.shape[1]
                d.partials, d.partial_chunks = part.data_ptr(), part.shape[0]
                out.append((mat, None))
                continue
            a, b = m["a"], m["b"]
            if a.stride(1) != 1 or b.stride(1) != 1 or a.shape[0] != b.shape[0]:
                raise EnerfError("gemm_wgrad_group: rows must be contiguous and of equal count")
            Ca, Cb = a.shape[1], m.get("Cb") or b.shape[1]
            gb = torch.empty((Ca,), dtype=torch.float32, device=a.device) if m.get("bias") else None
            if m.get("into") is not None:
                mat, c0 = m["into"]
                if mat.shape[0] != Ca or not mat.is_contiguous() or c0 + Cb > mat.shape[1]:
                    raise EnerfError("gemm_wgrad_group: `into` matrix does not hold the column block")
                gw, ptr, ldw = mat, mat.data_ptr() + 4 * c0, mat.shape[1]
            else:
                gw = torch.empty((Ca, Cb), dtype=torch.float32, device=a.device)
                ptr, ldw = gw.data_ptr(), Cb
            d.a, d.lda, d.Ca, d.b, d.ldb, d.Cb, d.P = a.data_ptr(), a.stride(0), Ca, b.data_ptr(), b.stride(0), Cb, a.shape[0]
            d.grad_w, d.ldw, d.grad_bias = ptr, ldw, _ptr(gb)
            out.append((gw, gb))
        a0 = next(m["a"] for m in members if m.get("partials") is None)
        ws = self._scratch(self.dll.enerf_gemm_wgrad_group_workspace_bytes(descs, n), a0.device)
        self._check(self.dll.enerf_gemm_wgrad_group(descs, n, ws.data_ptr(), ws.numel(), self.stream_of(a0)), "gemm_wgrad_group")
        return out

    def nerf_mlp_fwd(self, vox, x, packed, S, F):
        raw = torch.empty((vox.shape[0], 4), dtype=torch.float32, device=vox.device)
        self._check(self.dll.enerf_nerf_mlp_fwd(_ptr(vox), _ptr(x), _ptr(packed), vox.shape[0], S, F, _ptr(raw),
                                                self.stream_of(vox)), "nerf_mlp_fwd")
        return raw

    def nerf_mlp_bwd(self, vox, x, g_raw, packed, bimg, offsets, S, F, level=0):
        """Fused MLP backward (enerf_nerf_mlp_bwd) -> (g_vox, g_x, saves: list of 16 tensors).  ``level`` 1 / 2 (F = 11; 2: S <= 3): the
        weight gradients of the per-view colour (and aggregation) branch are accumulated in the kernel (enerf_nerf_mlp_bwd_partials): the
        saves they replace are None and a dict of per-wave partial sums follows — "q" (chunks, 4, 256), "rows" (chunks, 128) and, level 2,
        "g" (chunks, 2, 256), "v" (chunks, 1, 256)."""
        P, dev = vox.shape[0], vox.device
        E = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)
        g_vox, g_x = E(P, 8), E(P, S, F + 4)
        skip = () if level == 0 else ((2, 6, 7) if level == 1 else (2, 6, 7, 3, 4, 12, 13, 15))
        shapes = [(P, 88), (P, 32), (P, S, 64), (P, S, 32), (P, S, F), (P, 2 * F),
                  (P, S), (P, S, 64), (P, 64), (P,), (P, 64), (P, 16), (P, S), (P, S, 32), (P, 32), (P, S, F)]
        saves = [None if i in skip else E(*sh) for i, sh in enumerate(shapes)]
        a = MlpBwdArgs(_ptr(vox), _ptr(x), _ptr(g_raw), _ptr(packed), _ptr(bimg), _ptr(g_vox), _ptr(g_x))
        for i, t in enumerate(saves):
            a.save[i] = _ptr(t)
        a.P, a.F, a.S = P, F, S
        for i, o in enumerate(offsets):
            a.image_offsets[i] = int(o)
        if level == 0:
            self._check(self.dll.enerf_nerf_mlp_bwd(C.byref(a), self.stream_of(vox)), "nerf_mlp_bwd")
            return g_vox, g_x, saves
        chunks = int(self.dll.enerf_nerf_mlp_bwd_chunks(P))
        part = {"q": E(chunks, 4, 256), "rows": E(chunks, 128)}
        if level == 2:
            part["g"], part["v"] = E(chunks, 2, 256), E(chunks, 1, 256)
        self._check(self.dll.enerf_nerf_mlp_bwd_partials(C.byref(a), level, _ptr(part["q"]), _ptr(part.get("g")), _ptr(part.get("v")),
                                                         _ptr(part["rows"]), self.stream_of(vox)), "nerf_mlp_bwd_partials")
        return g_vox, g_x, saves, part

    def colsum(self, part):
        """out[i] = sum_c part[c, i] in a fixed order (enerf_colsum): the second stage of per-wave partial sums."""
        chunks, n = part.shape
        out = torch.empty((n,), dtype=torch.float32, device=part.device)
        self._check(self.dll.enerf_colsum(_ptr(part), chunks, n, _ptr(out), self.stream_of(part)), "colsum")
        return out

    def _gather_args(self, xyz, dn, uv, tex_cl, vol_cl, cam, tcen):
        B, P = xyz.shape[0], xyz.shape[1]
        a = GatherArgs(_ptr(xyz), _ptr(dn), _ptr(uv), _ptr(tex_cl), _ptr(vol_cl), _ptr(cam), _ptr(tcen))
        a.P, a.B, a.S, a.F = P, B, tex_cl.shape[1], tex_cl.shape[4]
        a.Hr, a.Wr = tex_cl.shape[2], tex_cl.shape[3]
        a.D, a.h, a.w = vol_cl.shape[1], vol_cl.shape[2], vol_cl.shape[3]
        assert vol_cl.shape[4] == 8 and cam.shape[-1] == 16 and tcen.shape[-1] == 4
        return a

    def gather_fwd(self, xyz, dn, uv, tex_cl, vol_cl, cam, tcen):
        """Training-path feature fetch (enerf_gather_fwd): xyz (B,P,3), dn (B,P), uv (B,P,2), tex_cl (B,S,Hr,Wr,F),
        vol_cl (B,D,h,w,8), cam (B,S,16), tcen (B,4) -> x (B,P,S,F+4), vox (B,P,8)."""
        a = self._gather_args(xyz, dn, uv, tex_cl, vol_cl, cam, tcen)
        x = torch.empty((a.B, a.P, a.S, a.F + 4), dtype=torch.float32, device=xyz.device)
        vox = torch.empty((a.B, a.P, 8), dtype=torch.float32, device=xyz.device)
        a.x, a.vox = _ptr(x), _ptr(vox)
        self._check(self.dll.enerf_gather_fwd(C.byref(a), self.stream_of(xyz)), "gather_fwd")
        return x, vox

    def gather_bwd(self, xyz, dn, uv, tex_cl, vol_cl, cam, tcen, g_x, g_vox, n_samples=0, ray_w=0):
        """-> (g_tex_cl, g_vol_cl, g_xyz, g_dn).  ``n_samples`` / ``ray_w``: raster hints (enerf_gather_args_t)."""
        a = self._gather_args(xyz, dn, uv, tex_cl, vol_cl, cam, tcen)
        a.n_samples, a.ray_w = int(n_samples), int(ray_w)
        E = lambda ref: torch.empty_like(ref)
        g_xyz, g_dn = E(xyz), E(dn)
        # the two scatter targets back to back: the library zeroes them with one launch (gather.hip zero_async2)
        # (when the first keeps the second 256-byte aligned; otherwise two allocations, two launches)
        if tex_cl.numel() % 64 == 0:
            acc = torch.empty((tex_cl.numel() + vol_cl.numel(),), dtype=torch.float32, device=xyz.device)
            g_tex, g_vol = acc[:tex_cl.numel()].view(tex_cl.shape), acc[tex_cl.numel():].view(vol_cl.shape)
        else:
            g_tex, g_vol = E(tex_cl), E(vol_cl)
        a.g_x, a.g_vox, a.g_tex, a.g_vol, a.g_xyz, a.g_dn = (_ptr(g_x), _ptr(g_vox), _ptr(g_tex), _ptr(g_vol), _ptr(g_xyz),
                                                            _ptr(g_dn))
        self._check(self.dll.enerf_gather_bwd(C.byref(a), self.stream_of(xyz)), "gather_bwd")
        return g_tex, g_vol, g_xyz, g_dn

    def conv_wgrad_cl(self, a_cl, b_cl, stride):
        """3x3x3 weight gradient from channels-last tensors a (n,Da,Ha,Wa,Ca), b (n,Db,Hb,Wb,Cb) -> (Ca,Cb,3,3,3)."""
        n, Da, Ha, Wa, Ca = a_cl.shape
        _, Db, Hb, Wb, Cb = b_cl.shape
        gw = torch.empty((Ca, Cb, 3, 3, 3), dtype=torch.float32, device=a_cl.device)
        ws = self._scratch(self.dll.enerf_conv_wgrad_workspace_bytes(n * Da * Ha * Wa, Ca, Cb, 3, 3, 3), a_cl.device)
        self._check(self.dll.enerf_conv_wgrad(_ptr(a_cl), _ptr(b_cl), n, Da, Ha, Wa, Ca, Db, Hb, Wb, Cb, 3, 3, 3, int(stride),
                                              1, 1, 1, _ptr(gw), ws.data_ptr(), ws.numel(), self.stream_of(a_cl)), "conv_wgrad")
        return gw

    def conv_wgrad_cl2d(self, a_cl, b_cl, k, stride):
        """k x k weight gradient (padding (k-1)/2) from channels-last 2-D tensors a (n,Ha,Wa,Ca), b (n,Hb,Wb,Cb) -> (Ca,Cb,k,k)."""
        n, Ha, Wa, Ca = a_cl.shape
        _, Hb, Wb, Cb = b_cl.shape
        p = (k - 1) // 2
        gw = torch.empty((Ca, Cb, k, k), dtype=torch.float32, device=a_cl.device)
        ws = self._scratch(self.dll.enerf_conv_wgrad_workspace_bytes(n * Ha * Wa, Ca, Cb, 1, k, k), a_cl.device)
        self._check(self.dll.enerf_conv_wgrad(_ptr(a_cl), _ptr(b_cl), n, 1, Ha, Wa, Ca, 1, Hb, Wb, Cb, 1, k, k, int(stride),
                                              0, p, p, _ptr(gw), ws.data_ptr(), ws.numel(), self.stream_of(a_cl)), "conv_wgrad")
        return gw

    def conv_wgrad(self, a, b, kernel, stride, padding, bias=False):
        """Weight gradient on the matrix cores (enerf_conv_wgrad).  ``a`` (n,Ca,*grid_a), ``b`` (n,Cb,*grid_b) in torch's
        channels-first layout (converted to channels-last here by the library's own adapter kernel); 2-D or 3-D.
        Returns (Ca, Cb, *kernel); with ``bias`` also the per-channel sums of ``a`` (the bias gradient when a = d y)."""
        nd = a.dim() - 2
        ga, gb = list(a.shape[2:]), list(b.shape[2:])
        if nd == 2:
            ga, gb, kernel, padding = [1] + ga, [1] + gb, (1,) + tuple(kernel), (0,) + tuple(padding)
        n, Ca, Cb = a.shape[0], a.shape[1], b.shape[1]
        pa, pb = ga[0] * ga[1] * ga[2], gb[0] * gb[1] * gb[2]
        a_cl = self.channels_last(a.contiguous().reshape(n, Ca, pa), n, Ca, pa)
        b_cl = self.channels_last(b.contiguous().reshape(n, Cb, pb), n, Cb, pb)
        gw = torch.empty((Ca, Cb) + tuple(kernel), dtype=torch.float32, device=a.device)
        ws = self._scratch(self.dll.enerf_conv_wgrad_workspace_bytes(n * pa, Ca, Cb, kernel[0], kernel[1], kernel[2]), a.device)
        self._check(self.dll.enerf_conv_wgrad(_ptr(a_cl), _ptr(b_cl), n, ga[0], ga[1], ga[2], Ca, gb[0], gb[1], gb[2], Cb,
                                              kernel[0], kernel[1], kernel[2], int(stride), padding[0], padding[1], padding[2],
                                              _ptr(gw), ws.data_ptr(), ws.numel(), self.stream_of(a)), "conv_wgrad")
        gw = gw if nd == 3 else gw.reshape(Ca, Cb, kernel[1], kernel[2])
        if not bias:
            return gw
        # the layer's bias gradient = per-channel sums of ``a`` (= d y), from the channels-last copy made above
        # enerf_channel_sums handles C <= 64 with C/4 dividing 256 (capi.hip); any other width takes the torch reduction
        fits = Ca % 4 == 0 and Ca <= 64 and 256 % (Ca // 4) == 0
        gb = self.channel_sums(a_cl, a_cl)[0].float() if fits else a.sum(dim=[0] + list(range(2, a.dim())))
        return gw, gb

    # -- ABI v7: the rest of the training step on the device (train_glue.hip) ----------------------------------------------
    def conv2d_s2k5_dgrad(self, w, dz, add=None):
        """Input gradient of Conv2d(cin -> cout, k5, s2, p2): w (cout,cin,5,5), dz (N,Ho,Wo,cout) -> (N,2Ho,2Wo,cin) (+ add)."""
        cout, cin = w.shape[0], w.shape[1]
        N, Ho, Wo, _ = dz.shape
        gx = torch.empty((N, 2 * Ho, 2 * Wo, cin), dtype=torch.float32, device=dz.device)
        ws = self._scratch(self.dll.enerf_conv2d_s2k5_dgrad_workspace_bytes(cin, cout, N, Ho, Wo), dz.device)
        self._check(self.dll.enerf_conv2d_s2k5_dgrad(_ptr(w), cin, cout, _ptr(dz), _ptr(add), _ptr(gx), N, Ho, Wo, ws.data_ptr(),
                                                     ws.numel(), self.stream_of(dz)), "conv2d_s2k5_dgrad")
        return gx

    def conv2d_s2k5_dgrad_pack(self, w):
        """The packed sub-kernel images of conv2d_s2k5_dgrad alone -> (packed (zero slack), parts, floats per part incl. slack,
        floats per part, output channels per part)."""
        cout, cin = w.shape[0], w.shape[1]
        total = self.dll.enerf_conv2d_s2k5_dgrad_packed_floats(cin, cout)
        cout3 = 2 * cin if 4 * cin > 32 else 4 * cin
        parts = 4 * cin // cout3
        packed = torch.zeros((total,), dtype=torch.float32, device=w.device)
        w3 = torch.empty((4 * cin * cout * 9,), dtype=torch.float32, device=w.device)
        self._check(self.dll.enerf_conv2d_s2k5_dgrad_pack(_ptr(w.contiguous()), cin, cout, _ptr(w3), _ptr(packed), self.stream_of(w)),
                    "conv2d_s2k5_dgrad_pack")
        return packed, parts, total // parts, self.dll.enerf_conv2d_layer_packed_floats(cout, cout3, 3), cout3

    def conv2d_s2k5_dgrad_packed(self, packed, cin, cout, dz, add=None):
        """conv2d_s2k5_dgrad on images prepared by conv2d_s2k5_dgrad_pack (or a PackPlan's gather)."""
        N, Ho, Wo, _ = dz.shape
        gx = torch.empty((N, 2 * Ho, 2 * Wo, cin), dtype=torch.float32, device=dz.device)
        ws = self._scratch(self.dll.enerf_conv2d_s2k5_dgrad_workspace_bytes(cin, cout, N, Ho, Wo), dz.device)
        self._check(self.dll.enerf_conv2d_s2k5_dgrad_packed(_ptr(packed), cin, cout, _ptr(dz), _ptr(add), _ptr(gx), N, Ho, Wo, ws.data_ptr(),
                                                            ws.numel(), self.stream_of(dz)), "conv2d_s2k5_dgrad_packed")
        return gx

    def resize_ac_adjoint(self, g_fine, Hc, Wc, add=None):
        """(..., Hf, Wf) planar gradient maps -> (..., Hc, Wc): adjoint of the align-corners bilinear resize."""
        lead, (Hf, Wf) = g_fine.shape[:-2], g_fine.shape[-2:]
        out = torch.empty(tuple(lead) + (Hc, Wc), dtype=torch.float32, device=g_fine.device)
        self._check(self.dll.enerf_resize_ac_adjoint(_ptr(g_fine), _ptr(add), g_fine.numel() // (Hf * Wf), Hf, Wf, Hc, Wc, _ptr(out),
                                                     self.stream_of(g_fine)), "resize_ac_adjoint")
        return out

    def get_depth_values_bwd(self, prev_depth, prev_std, prev_nf, g_dv, depth_inv):
        """-> (g_depth, g_std) (B,hp,wp): views of one (2,B,hp,wp) buffer."""
        B, D, h, w = g_dv.shape
        hp, wp = prev_depth.shape[-2:]
        g = torch.empty((2, B, hp, wp), dtype=torch.float32, device=g_dv.device)
        scratch = torch.empty((2, B, h, w), dtype=torch.float32, device=g_dv.device)
        self._check(self.dll.enerf_get_depth_values_bwd(_ptr(prev_depth), _ptr(prev_std), _ptr(prev_nf), _ptr(g_dv), B, D, h, w, hp, wp,
                                                        int(depth_inv), _ptr(g), g[1].data_ptr(), _ptr(scratch), self.stream_of(g_dv)),
                    "get_depth_values_bwd")
        return g[0], g[1]

    def ray_samples_fwd(self, rays8, depth, std, nf, Ns, Hr, Wr, depth_inv, want_rays12=False):
        """build_rays + sample_along_depth -> z (B,N,Ns), xyz (B,N,Ns,3), dn (B,N,Ns), uv (B,N,Ns,2)[, rays12 (B,N,12)]."""
        B, N = rays8.shape[:2]
        h, w = depth.shape[-2:]
        E = lambda *sh: torch.empty(sh, dtype=torch.float32, device=rays8.device)
        z, xyz, dn, uv = E(B, N, Ns), E(B, N, Ns, 3), E(B, N, Ns), E(B, N, Ns, 2)
        r12 = E(B, N, 12) if want_rays12 else None
        self._check(self.dll.enerf_ray_samples_fwd(_ptr(rays8), _ptr(depth), _ptr(std), _ptr(nf), B, N, Ns, h, w, Hr, Wr, int(depth_inv),
                                                   _ptr(z), _ptr(xyz), _ptr(dn), _ptr(uv), _ptr(r12), self.stream_of(rays8)),
                    "ray_samples_fwd")
        return (z, xyz, dn, uv, r12) if want_rays12 else (z, xyz, dn, uv)

    def ray_samples_bwd(self, rays8, depth, std, nf, g_xyz, g_dn, Ns, Hr, Wr, depth_inv):
        B, N = rays8.shape[:2]
        h, w = depth.shape[-2:]
        g = torch.empty((2, B, h, w), dtype=torch.float32, device=rays8.device)
        self._check(self.dll.enerf_ray_samples_bwd(_ptr(rays8), _ptr(depth), _ptr(std), _ptr(nf), _ptr(g_xyz), _ptr(g_dn), B, N, Ns, h, w,
                                                   Hr, Wr, int(depth_inv), _ptr(g), g[1].data_ptr(), self.stream_of(rays8)),
                    "ray_samples_bwd")
        return g[0], g[1]

    def camera_tables(self, src_ixts, src_exts, tar_ext, render_scale):
        B, S = src_exts.shape[:2]
        cam = torch.empty((B, S, 16), dtype=torch.float32, device=src_exts.device)
        tcen = torch.empty((B, 4), dtype=torch.float32, device=src_exts.device)
        self._check(self.dll.enerf_camera_tables(_ptr(src_ixts), _ptr(src_exts), _ptr(tar_ext), B, S, float(render_scale), _ptr(cam),
                                                 _ptr(tcen), self.stream_of(src_exts)), "camera_tables")
        return cam, tcen

    def weights_flip_transpose(self, w):
        """w (cout,cin,*k) -> (cin,cout,*k) with every spatial axis reversed: the dgrad weights of a stride-1 convolution."""
        cout, cin = w.shape[:2]
        taps = w.numel() // (cout * cin)
        out = torch.empty((cin, cout) + tuple(w.shape[2:]), dtype=torch.float32, device=w.device)
        self._check(self.dll.enerf_weights_flip_transpose(_ptr(w), cout, cin, taps, _ptr(out), self.stream_of(w)), "weights_flip_transpose")
        return out

    def concat2_pad(self, a, b, n):
        out = torch.empty((n,), dtype=torch.float32, device=a.device)
        self._check(self.dll.enerf_concat2_pad(_ptr(a), a.numel(), _ptr(b), 0 if b is None else b.numel(), n, _ptr(out), self.stream_of(a)),
                    "concat2_pad")
        return out

    def pack_texels_train(self, feat_cl, src_inps, Hr, Wr):
        """feat_cl (n,Hr,Wr,C) channels-last, src_inps (n,3,H,W) -> tex (n,Hr,Wr,C+3)."""
        n, _, _, Cc = feat_cl.shape
        H, W = src_inps.shape[-2:]
        tex = torch.empty((n, Hr, Wr, Cc + 3), dtype=torch.float32, device=feat_cl.device)
        self._check(self.dll.enerf_pack_texels_train(_ptr(feat_cl), Cc, _ptr(src_inps), H, W, Hr, Wr, n, _ptr(tex), self.stream_of(tex)),
                    "pack_texels_train")
        return tex

    def slice_channels(self, src, c0, Cc):
        F = src.shape[-1]
        dst = torch.empty(tuple(src.shape[:-1]) + (Cc,), dtype=torch.float32, device=src.device)
        self._check(self.dll.enerf_slice_channels(_ptr(src), src.numel() // F, F, c0, Cc, _ptr(dst), self.stream_of(src)), "slice_channels")
        return dst

    def concat_channels(self, a, b, Cc):
        """a (..., Ca), b (..., Cb) or None -> (..., Cc) = [a | b | 0]."""
        Ca, Cb = a.shape[-1], 0 if b is None else b.shape[-1]
        out = torch.empty(tuple(a.shape[:-1]) + (Cc,), dtype=torch.float32, device=a.device)
        self._check(self.dll.enerf_concat_channels(_ptr(a), Ca, _ptr(b), Cb, a.numel() // Ca, Cc, _ptr(out), self.stream_of(a)),
                    "concat_channels")
        return out

    def gather_images(self, srcs, which, idx):
        """out[i] = idx[i] >= 0 ? srcs[which[i]].flatten()[idx[i]] : 0; srcs: <= 64 contiguous float tensors; which/idx int32."""
        arr = (C.c_void_p * len(srcs))(*[_ptr(t) for t in srcs])
        out = torch.empty((idx.numel(),), dtype=torch.float32, device=idx.device)
        self._check(self.dll.enerf_gather_images(C.cast(arr, C.c_void_p), len(srcs), which.data_ptr(), idx.data_ptr(), idx.numel(), _ptr(out),
                                                 self.stream_of(out)), "gather_images")
        return out

    def cast_f32(self, x64):
        out = torch.empty(x64.shape, dtype=torch.float32, device=x64.device)
        self._check(self.dll.enerf_cast_f64_f32(x64.data_ptr(), x64.numel(), _ptr(out), self.stream_of(out)), "cast_f64_f32")
        return out

    def reciprocal(self, x):
        out = torch.empty_like(x)
        self._check(self.dll.enerf_reciprocal(_ptr(x), x.numel(), _ptr(out), self.stream_of(x)), "reciprocal")
        return out

    def add(self, a, b):
        out = torch.empty_like(a)
        self._check(self.dll.enerf_add(_ptr(a), _ptr(b), a.numel(), _ptr(out), self.stream_of(a)), "add")
        return out

    def composite(self, raw, z, white_bkgd=False):
        n, Ns = z.shape
        rgb = torch.empty((n, 3), dtype=torch.float32, device=raw.device)
        depth = torch.empty((n,), dtype=torch.float32, device=raw.device)
        weights = torch.empty((n, Ns), dtype=torch.float32, device=raw.device)
        self._check(self.dll.enerf_composite(_ptr(raw), _ptr(z), n, Ns, int(white_bkgd), _ptr(rgb), _ptr(depth), _ptr(weights),
                                             self.stream_of(raw)), "composite")
        return rgb, depth, weights

    def composite_bwd(self, raw, z, g_rgb, g_depth, g_weights):
        n, Ns = z.shape
        g_raw, g_z = torch.empty_like(raw), torch.empty_like(z)
        self._check(self.dll.enerf_composite_bwd(_ptr(raw), _ptr(z), _ptr(g_rgb), _ptr(g_depth), _ptr(g_weights), n, Ns,   # None = zeros
                                                 _ptr(g_raw), _ptr(g_z), self.stream_of(raw)), "composite_bwd")
        return g_raw, g_z

    # -- whole frame / mask compaction -------------------------------------------------------------
    def mask_compact(self, mask: torch.Tensor, workspace=None):
        """network_human.py:90-93 on device: (index int32 (n), count int32 (1)) of the non-zero mask elements."""
        if not mask.is_contiguous():
            raise EnerfError("mask must be contiguous")
        n = mask.numel()
        dev = mask.device
        need = self.dll.enerf_mask_compact_workspace_bytes(n)
        if workspace is None or workspace.numel() * 4 < need:
            workspace = torch.empty(((need + 3) // 4,), dtype=torch.int32, device=dev)
        index = torch.empty((n,), dtype=torch.int32, device=dev)
        count = torch.empty((1,), dtype=torch.int32, device=dev)
        self._check(self.dll.enerf_mask_compact(mask.data_ptr(), mask.element_size(), n, index.data_ptr(), count.data_ptr(),
                                                workspace.data_ptr(), workspace.numel() * 4, self.stream_of(mask)),
                    "mask_compact")
        return index, count

    def forward_workspace_bytes(self, args: "FrameArgs") -> int:
        n = self.dll.enerf_forward_workspace_bytes(C.byref(args))
        if n == 0:
            raise EnerfError(f"forward: {self.dll.enerf_last_error().decode()}")
        return n

    def forward(self, args: "FrameArgs", stream):
        self._check(self.dll.enerf_forward(C.byref(args), stream), "forward")

    # -- source-view cache (enerf_amd/source_cache.py owns the tensors) -----------------------------------
    def source_cache_sizes(self, cas: "Cascade", V: int, H: int, W: int):
        """(l2_stride, floats per buffer [feat_l0, feat_l1, feat_l2, tex_0.., exts, ixts]) of a cache for this cascade."""
        l2s = _i(0)
        floats = (_ll * SOURCE_CACHE_BUFFERS)()
        self._check(self.dll.enerf_source_cache_sizes(C.byref(cas), V, H, W, C.byref(l2s), floats), "source_cache_sizes")
        return l2s.value, list(floats)

    def source_cache_build_workspace(self, H: int, W: int, device):
        """The build's scratch (the FeatureNet workspace of 4 images): a caller that rebuilds keeps one and passes it back in."""
        nb = self.dll.enerf_source_cache_build_workspace_bytes(H, W)
        return torch.empty(((nb + 3) // 4,), dtype=torch.float32, device=device)

    def source_cache_build(self, cache: "SourceCacheStruct", src_inps, exts, ixts, packed, cas: "Cascade", chunk=0, options=None,
                           workspace=None):
        """FeatureNet + texel packing of ``src_inps`` (V,3,H,W) into the cache's buffers, ``chunk`` (<= 4) images at a time."""
        ws = workspace if workspace is not None else self.source_cache_build_workspace(cache.H, cache.W, src_inps.device)
        self._check(self.dll.enerf_source_cache_build(C.byref(cache), _ptr(src_inps), _ptr(exts), _ptr(ixts), _ptr(packed),
                                                      C.byref(cas), int(chunk), ws.data_ptr(), ws.numel() * 4, _opt(options),
                                                      self.stream_of(src_inps)), "source_cache_build")

    def forward_cached_workspace_bytes(self, args: "FrameArgs", cache: "SourceCacheStruct") -> int:
        n = self.dll.enerf_forward_cached_workspace_bytes(C.byref(args), C.byref(cache))
        if n == 0:
            raise EnerfError(f"forward_cached: {self.dll.enerf_last_error().decode()}")
        return n

    def forward_cached(self, args: "FrameArgs", cache: "SourceCacheStruct", view_idx_ptr, stream):
        """``view_idx_ptr``: address of the (B,S) int32 DEVICE array (never read on the host)."""
        self._check(self.dll.enerf_forward_cached(C.byref(args), C.byref(cache), view_idx_ptr, stream), "forward_cached")

    # -- the steps before / after the path ---------------------------------
    def gen_rays(self, tar_ext, tar_ixt, Hr, Wr, scale, out=None):
        """lib/datasets/enerf_utils.py:61-71 (full image) on device -> (B, Hr*Wr, 8)."""
        B = tar_ext.shape[0]
        rays = _out(out, (B, Hr * Wr, 8), tar_ext.device, "gen_rays")
        self._check(self.dll.enerf_gen_rays(_ptr(tar_ext), _ptr(tar_ixt), B, Hr, Wr, float(scale), _ptr(rays),
                                            self.stream_of(rays)), "gen_rays")
        return rays

    def pack_rgb8(self, rgb, H, W, flip=True):
        """gui_human.py:88-91: (H*W,3) float in [0,1] -> (H,W,3) uint8, vertically flipped for GL."""
        out = torch.empty((H, W, 3), dtype=torch.uint8, device=rgb.device)
        self._check(self.dll.enerf_pack_rgb8(_ptr(rgb), H, W, int(flip), out.data_ptr(), self.stream_of(rgb)),
                    "pack_rgb8")
        return out

    def gen_rays_at(self, tar_ext, tar_ixt, xy, scale):
        """lib/datasets/enerf_utils.py:45-56 (training branch) for the pixel list ``xy`` (B,N,2) int32 -> (B,N,8)."""
        B, N = xy.shape[:2]
        if xy.dtype != torch.int32 or not xy.is_contiguous():
            raise EnerfError("xy must be a contiguous int32 tensor (B,N,2)")
        rays = torch.empty((B, N, 8), dtype=torch.float32, device=tar_ext.device)
        self._check(self.dll.enerf_gen_rays_at(_ptr(tar_ext), _ptr(tar_ixt), xy.data_ptr(), B, N, float(scale), _ptr(rays),
                                               self.stream_of(rays)), "gen_rays_at")
        return rays

    def rays_bbox_mask(self, rays, bounds):
        """lib/utils/net_utils.py:13-28 gen_rays_bbox: rays (N,8), bounds (2,3) -> int32 mask (N)."""
        n = rays.shape[0]
        mask = torch.empty((n,), dtype=torch.int32, device=rays.device)
        self._check(self.dll.enerf_rays_bbox_mask(_ptr(rays), _ptr(bounds), n, mask.data_ptr(), self.stream_of(rays)),
                    "rays_bbox_mask")
        return mask

    def select_views(self, cam_points, c2w, k):
        """zjumocap/enerf_interactive.py:207-210: indices (k) int32 of the cameras nearest to the target camera."""
        idx = torch.empty((k,), dtype=torch.int32, device=cam_points.device)
        self._check(self.dll.enerf_select_views(_ptr(cam_points), cam_points.shape[0], _ptr(c2w), k, idx.data_ptr(),
                                                self.stream_of(cam_points)), "select_views")
        return idx

    def gather_views(self, inps, exts, ixts, idx):
        """:214-217: inps (V,H,W,3), exts (V,4,4), ixts (V,3,3) + idx (k) -> src_inps (k,3,H,W), src_exts, src_ixts."""
        V, H, W, _ = inps.shape
        k, dev = idx.numel(), inps.device
        si = torch.empty((k, 3, H, W), dtype=torch.float32, device=dev)
        se = torch.empty((k, 4, 4), dtype=torch.float32, device=dev)
        sk = torch.empty((k, 3, 3), dtype=torch.float32, device=dev)
        self._check(self.dll.enerf_gather_views(_ptr(inps), _ptr(exts), _ptr(ixts), idx.data_ptr(), k, H, W, _ptr(si),
                                                _ptr(se), _ptr(sk), self.stream_of(inps)), "gather_views")
        return si, se, sk

    def ingest_views_u8(self, img, mask=None, dilate=0, out=None):
        """zjumocap/enerf_interactive.py:116-124,135 + :145 on the device: img (V,H,W,3) uint8, mask (V,H,W) uint8 / bool or None
        -> (V,3,H,W) float32 in [-1,1], masked-out pixels (after a ``dilate`` x ``dilate`` box dilation of ``mask != 0``) at -1."""
        if img.dtype != torch.uint8 or img.dim() != 4 or img.shape[-1] != 3 or not img.is_contiguous():
            raise EnerfError(f"ingest_views_u8: img must be a contiguous uint8 (V,H,W,3) tensor, got {img.dtype} {tuple(img.shape)}")
        V, H, W, _ = img.shape
        if mask is not None:
            if mask.dtype not in (torch.uint8, torch.bool) or tuple(mask.shape) != (V, H, W) or not mask.is_contiguous() \
                    or mask.device != img.device:
                raise EnerfError(f"ingest_views_u8: mask must be a contiguous uint8 / bool ({V},{H},{W}) tensor on the image's device")
        if out is None:
            out = torch.empty((V, 3, H, W), dtype=torch.float32, device=img.device)
        elif tuple(out.shape) != (V, 3, H, W) or out.device != img.device:
            raise EnerfError(f"ingest_views_u8: out must be ({V},3,{H},{W}) on the image's device")
        self._check(self.dll.enerf_ingest_views_u8(img.data_ptr(), None if mask is None else mask.data_ptr(), int(dilate), V, H, W,
                                                   _ptr(out), self.stream_of(img)),
                    "ingest_views_u8")
        return out

    def ingest_raw_geometry(self, Hraw, Wraw, input_ratio=1.0):
        """(Hs, Ws) of a raw Hraw x Wraw frame resized by ``input_ratio``: rounded half-to-even, the C side's one rounding."""
        hs, ws = C.c_int(0), C.c_int(0)
        self._check(self.dll.enerf_ingest_raw_geometry(int(Hraw), int(Wraw), float(input_ratio), C.byref(hs), C.byref(ws)),
                    "ingest_raw_geometry")
        return hs.value, ws.value

    def ingest_raw_u8(self, img, ixts=None, dist=None, mask=None, dilate=0, input_ratio=1.0, crop=None, scratch=None, out=None,
                      mask_out=None):
        """Raw camera frames to the caches' float image on the device (zjumocap/enerf_interactive.py:116-135, enerf_outdoor/enerf.py:
        129-152): img (V,Hraw,Wraw,3) uint8, ixts (V,3,3) and dist (V,5) = (k1,k2,p1,p2,k3) float32 (dist None: no undistortion),
        mask (V,Hraw,Wraw) uint8 / bool or None, ``crop`` = (y0, x0, H, W) in the image resized by ``input_ratio`` (None: all of it)
        -> (V,3,H,W) float32 in [-1,1]; ``mask_out`` (V,H,W) uint8 receives the final mask.  ``scratch`` (V,Hraw,Wraw) uint8 holds the
        dilated raw mask (allocated here when a mask is dilated and none is given)."""
        if img.dtype != torch.uint8 or img.dim() != 4 or img.shape[-1] != 3 or not img.is_contiguous():
            raise EnerfError(f"ingest_raw_u8: img must be a contiguous uint8 (V,Hraw,Wraw,3) tensor, got {img.dtype} {tuple(img.shape)}")
        V, Hraw, Wraw, _ = img.shape
        dev = img.device
        for name, t, shape in (("ixts", ixts, (V, 3, 3)), ("dist", dist, (V, 5))):
            if t is not None and (t.dtype != torch.float32 or tuple(t.shape) != shape or not t.is_contiguous() or t.device != dev):
                raise EnerfError(f"ingest_raw_u8: {name} must be a contiguous float32 {shape} tensor on the image's device")
        if dist is not None and ixts is None:
            raise EnerfError("ingest_raw_u8: dist needs ixts")
        for name, t in (("mask", mask), ("scratch", scratch)):
            if t is not None and (t.dtype not in (torch.uint8, torch.bool) or tuple(t.shape) != (V, Hraw, Wraw) or not t.is_contiguous()
                                  or t.device != dev or (name == "scratch" and t.dtype != torch.uint8)):
                raise EnerfError(f"ingest_raw_u8: {name} must be a contiguous uint8{' / bool' if name == 'mask' else ''} "
                                 f"({V},{Hraw},{Wraw}) tensor on the image's device")
        if crop is None:
            y0, x0 = 0, 0
            H, W = self.ingest_raw_geometry(Hraw, Wraw, input_ratio)
        else:
            y0, x0, H, W = (int(c) for c in crop)
        if mask is not None and dilate and scratch is None:
            scratch = torch.empty((V, Hraw, Wraw), dtype=torch.uint8, device=dev)
        if out is None:
            out = torch.empty((V, 3, H, W), dtype=torch.float32, device=dev)
        elif tuple(out.shape) != (V, 3, H, W) or out.device != dev:
            raise EnerfError(f"ingest_raw_u8: out must be ({V},3,{H},{W}) on the image's device")
        if mask_out is not None and (mask_out.dtype != torch.uint8 or tuple(mask_out.shape) != (V, H, W) or not mask_out.is_contiguous()
                                     or mask_out.device != dev):
            raise EnerfError(f"ingest_raw_u8: mask_out must be a contiguous uint8 ({V},{H},{W}) tensor on the image's device")
        dp = lambda t: None if t is None else t.data_ptr()
        self._check(self.dll.enerf_ingest_raw_u8(img.data_ptr(), dp(mask), dp(ixts), dp(dist), V, Hraw, Wraw, float(input_ratio), y0, x0,
                                                 H, W, int(dilate), dp(scratch), _ptr(out), dp(mask_out), self.stream_of(img)),
                    "ingest_raw_u8")
        return out

    def vhull_workspace(self, n_layers=1, device="cpu"):
        """The accumulators of one ``vhull_bounds`` call in flight: ``enerf_vhull_workspace_bytes`` bytes as an int32 tensor."""
        a = VhullArgs(n_layers=int(n_layers))
        n = self.dll.enerf_vhull_workspace_bytes(C.byref(a))
        if n == 0:
            raise EnerfError(f"vhull_workspace failed: {self.dll.enerf_last_error().decode()}")
        return torch.empty(((n + 3) // 4,), dtype=torch.int32, device=device)

    def vhull_bounds(self, masks, exts, ixts, scene_bounds, grid=(128, 128, 128), n_layers=1, labels=False, min_views=2, max_miss=0,
                     pad=0.0, out=None, occupancy=None, workspace=None):
        """The foreground's world-space box per layer, carved from the masks (the model: include/enerf_hip.h, enerf_vhull_bounds):
        masks (V,H,W) uint8 / bool, exts (V,4,4) and ixts (V,3,3) float32 at the masks' resolution, all on one device;
        ``scene_bounds`` ((lo), (hi)) and ``grid`` (Gx,Gy,Gz) are HOST values (a sequence, an array or a CPU tensor).  Returns
        ``(bounds (L,2,3) float32, counts (L) int32, flags (L) int32, corners (L,8,3) float32)`` — ``out`` when given, the same four.
        ``occupancy`` (Gz,Gy,Gx) uint8 receives the voxels (bit l = layer l).  ``workspace``: :meth:`vhull_workspace`, the caller's
        own for calls on a stream of its own or under graph capture (allocated here otherwise).  Nothing is read back."""
        if masks.dtype == torch.bool:
            masks = masks.view(torch.uint8)
        if masks.dtype != torch.uint8 or masks.dim() != 3 or not masks.is_contiguous():
            raise EnerfError(f"vhull_bounds: masks must be a contiguous uint8 / bool (V,H,W) tensor, got {masks.dtype} {tuple(masks.shape)}")
        V, H, W = masks.shape
        dev = masks.device
        for name, t, shape in (("exts", exts, (V, 4, 4)), ("ixts", ixts, (V, 3, 3))):
            if t.dtype != torch.float32 or tuple(t.shape) != shape or not t.is_contiguous() or t.device != dev:
                raise EnerfError(f"vhull_bounds: {name} must be a contiguous float32 {shape} tensor on the masks' device")
        if isinstance(scene_bounds, torch.Tensor) and scene_bounds.device.type != "cpu":
            raise EnerfError("vhull_bounds: scene_bounds are host values (part of the plan), got a device tensor")
        sb = torch.as_tensor(scene_bounds, dtype=torch.float32).reshape(-1).tolist()
        grid = tuple(int(x) for x in grid)
        if len(sb) != 6 or len(grid) != 3:
            raise EnerfError("vhull_bounds: scene_bounds is ((x0,y0,z0),(x1,y1,z1)) and grid (Gx,Gy,Gz)")
        L = int(n_layers)
        shapes = ((L, 2, 3), (L,), (L,), (L, 8, 3))
        dtypes = (torch.float32, torch.int32, torch.int32, torch.float32)
        if out is None:
            out = tuple(torch.empty(s, dtype=d, device=dev) for s, d in zip(shapes, dtypes))
        else:
            out = tuple(out)
            names = ("bounds", "counts", "flags", "corners")
            if len(out) != 4:
                raise EnerfError("vhull_bounds: out is (bounds, counts, flags, corners)")
            for name, t, s, d in zip(names, out, shapes, dtypes):
                if tuple(t.shape) != s or t.dtype != d or not t.is_contiguous() or t.device != dev:
                    raise EnerfError(f"vhull_bounds: out {name} must be a contiguous {d} {s} tensor on the masks' device")
        if occupancy is not None and (occupancy.dtype != torch.uint8 or tuple(occupancy.shape) != grid[::-1] or not occupancy.is_contiguous()
                                      or occupancy.device != dev):
            raise EnerfError(f"vhull_bounds: occupancy must be a contiguous uint8 {grid[::-1]} tensor on the masks' device")
        if workspace is None:
            workspace = self.vhull_workspace(L, dev)
        elif workspace.device != dev or not workspace.is_contiguous():
            raise EnerfError("vhull_bounds: workspace must be a contiguous tensor on the masks' device")
        a = VhullArgs(masks=masks.data_ptr(), exts=exts.data_ptr(), ixts=ixts.data_ptr(), V=V, H=H, W=W, n_layers=L, labels=int(bool(labels)),
                      min_views=int(min_views), max_miss=int(max_miss), pad=float(pad), bounds=out[0].data_ptr(), counts=out[1].data_ptr(),
                      flags=out[2].data_ptr(), corners=out[3].data_ptr(), occupancy=None if occupancy is None else occupancy.data_ptr(),
                      workspace=workspace.data_ptr(), workspace_bytes=workspace.numel() * workspace.element_size())
        for i in range(6):
            a.scene_bounds[i // 3][i % 3] = sb[i]
        for i in range(3):
            a.grid[i] = grid[i]
        self._check(self.dll.enerf_vhull_bounds(C.byref(a), self.stream_of(masks)), "vhull_bounds")
        return out

    def bounds_near_far(self, vertices, tar_ext, near_min=0.05):
        """zjumocap/enerf_interactive.py:198-201 without its two ``.item()``: vertices (n,3) or (B,n,3), tar_ext (B,4,4) ->
        near_far (B,2) = [max(min z, near_min), max z] of the vertices' camera-space depths."""
        B = tar_ext.shape[0]
        if tuple(tar_ext.shape) != (B, 4, 4) or vertices.shape[-1] != 3 or vertices.dim() not in (2, 3):
            raise EnerfError(f"bounds_near_far: vertices (n,3) / (B,n,3) and tar_ext (B,4,4), got {tuple(vertices.shape)} / {tuple(tar_ext.shape)}")
        if vertices.dim() == 2:
            vertices = vertices[None].expand(B, -1, -1)
        if vertices.shape[0] != B:
            raise EnerfError(f"bounds_near_far: {vertices.shape[0]} vertex sets for {B} cameras")
        vertices = vertices.contiguous()
        near_far = torch.empty((B, 2), dtype=torch.float32, device=tar_ext.device)
        self._check(self.dll.enerf_bounds_near_far(_ptr(vertices), vertices.shape[1], _ptr(tar_ext), B, float(near_min),
                                                   _ptr(near_far), self.stream_of(tar_ext)), "bounds_near_far")
        return near_far

    def eval_stats(self, pred_rgb, gt_rgb, mask=None, pred_depth=None, gt_depth=None, image_hw=None, crop=(0, 0),
                   sync=True):
        """evaluators/enerf.py:45-71,88-103 on device.  Returns dict(psnr[, abs, acc_2, acc_10]) after ONE 48-byte D2H
        copy — or, with ``sync=False``, the 6-double device accumulator (see include/enerf_hip.h)."""
        acc = torch.empty((6,), dtype=torch.float64, device=pred_rgb.device)
        n_rgb = pred_rgb.numel() // 3
        mb = 0
        if mask is not None:
            if mask.dtype not in (torch.int32, torch.uint8, torch.bool) or not mask.is_contiguous():
                raise EnerfError("mask must be a contiguous int32 / uint8 / bool tensor")
            mb = mask.element_size()
        n_d = 0 if pred_depth is None else pred_depth.numel()
        h, w = image_hw if image_hw is not None else (0, 0)
        self._check(self.dll.enerf_eval_stats(_ptr(pred_rgb), _ptr(gt_rgb), None if mask is None else mask.data_ptr(), mb,
                                              n_rgb, int(w), int(h), int(crop[0]), int(crop[1]), _ptr(pred_depth),
                                              _ptr(gt_depth), n_d, acc.data_ptr(), self.stream_of(pred_rgb)), "eval_stats")
        if not sync:
            return acc
        return stats_from_acc(acc.cpu().tolist())

    def eval_ssim(self, pred_rgb, gt_rgb, mask=None, image_hw=None, crop=(0, 0), bbox=False, mask_is_one=False, sync=True):
        """``ssim(gt, pred, multichannel=True)`` of evaluators/enerf.py:76 / enerf_human.py:66 (skimage 0.18: float64, 7x7 uniform
        window, data_range 2) on device, with the evaluators' preprocessing: pixels whose ``mask`` is off (``>= 1`` is on; ``== 1``
        with ``mask_is_one``) count as 0, and the image is the ``eval_center`` slice ``crop`` = (crop_h, crop_w) or, with ``bbox``,
        the bounding box of the on pixels.  ``pred_rgb`` / ``gt_rgb``: (B, h*w, 3) or (h*w, 3) with ``image_hw`` = (h, w); ``mask``
        (B, h*w).  Returns one float per image (NaN: empty or < 7 pixel bounding box) after ONE 16*B-byte D2H copy — or, with
        ``sync=False``, the (B,2) float64 device tensor {ssim, windows per channel}; nothing synchronises then."""
        if image_hw is None:
            raise EnerfError("eval_ssim needs image_hw=(h, w)")
        h, w = int(image_hw[0]), int(image_hw[1])
        if h <= 0 or w <= 0 or pred_rgb.numel() == 0 or pred_rgb.numel() % (h * w * 3) or gt_rgb.numel() != pred_rgb.numel():
            raise EnerfError(f"eval_ssim: pred / gt must be (B, {h}*{w}, 3) tensors of the same size")
        B = pred_rgb.numel() // (h * w * 3)
        mb = 0
        if mask is not None:
            if mask.dtype not in (torch.int32, torch.uint8, torch.bool) or not mask.is_contiguous():
                raise EnerfError("mask must be a contiguous int32 / uint8 / bool tensor")
            if mask.numel() != B * h * w:
                raise EnerfError(f"eval_ssim: mask has {mask.numel()} elements, the images {B * h * w} pixels")
            mb = mask.element_size()
        rect = 2 if bbox else (1 if (int(crop[0]), int(crop[1])) != (0, 0) else 0)
        ch, cw = (int(crop[0]), int(crop[1])) if rect == 1 else (0, 0)
        pp, gp = _ptr(pred_rgb), _ptr(gt_rgb)                          # dtype / contiguity checked before anything is sized
        nbytes = self.dll.enerf_eval_ssim_workspace_bytes(B, h, w, rect, ch, cw)
        if nbytes == 0:
            raise EnerfError(f"eval_ssim failed: {self.dll.enerf_last_error().decode()}")
        ws = torch.empty(((nbytes + 7) // 8,), dtype=torch.float64, device=pred_rgb.device)
        out = torch.empty((B, 2), dtype=torch.float64, device=pred_rgb.device)
        self._check(self.dll.enerf_eval_ssim(pp, gp, None if mask is None else mask.data_ptr(), mb, int(bool(mask_is_one)), B, h, w,
                                             rect, ch, cw, ws.data_ptr(), out.data_ptr(), self.stream_of(pred_rgb)), "eval_ssim")
        if not sync:
            return out
        return out.cpu()[:, 0].tolist()

    # -- evaluator LPIPS (csrc/lpips_vgg.h) ------------------------------------------------------------
    def lpips_pack(self, convs, lins):
        """``convs``: thirteen (w (cout,cin,3,3), b (cout)) pairs in trunk order, ``lins``: five (C_l) tensors -> the packed image
        ``enerf_eval_lpips`` reads (``enerf_amd.lpips.LpipsWeights`` builds these lists)."""
        if len(convs) != 13 or len(lins) != 5:
            raise EnerfError("lpips_pack needs 13 (w, b) pairs and 5 lin vectors")
        raw = LpipsRaw()
        for i, ((w, b), (cin, cout)) in enumerate(zip(convs, VGG_CONVS)):
            if tuple(w.shape) != (cout, cin, 3, 3) or tuple(b.shape) != (cout,):
                raise EnerfError(f"lpips_pack: conv {i} must be ({cout},{cin},3,3) + ({cout},), got {tuple(w.shape)} + {tuple(b.shape)}")
            raw.conv[i].w, raw.conv[i].b = _ptr(w), _ptr(b)
        for l, (v, c) in enumerate(zip(lins, LPIPS_TAP_CHANNELS)):
            if v.numel() != c:
                raise EnerfError(f"lpips_pack: lin{l} must hold {c} values, got {tuple(v.shape)}")
            raw.lin[l] = _ptr(v)
        dev = convs[0][0].device
        packed = torch.empty((self.dll.enerf_lpips_packed_floats(),), dtype=torch.float32, device=dev)
        self._check(self.dll.enerf_lpips_pack(C.byref(raw), _ptr(packed), self.stream_of(packed)), "lpips_pack")
        return packed

    def _lpips_args(self, what, pred_rgb, gt_rgb, mask, image_hw, crop, rect):
        if image_hw is None:
            raise EnerfError(f"{what} needs image_hw=(h, w)")
        h, w = int(image_hw[0]), int(image_hw[1])
        if h <= 0 or w <= 0 or pred_rgb.numel() == 0 or pred_rgb.numel() % (h * w * 3) or gt_rgb.numel() != pred_rgb.numel():
            raise EnerfError(f"{what}: pred / gt must be (B, {h}*{w}, 3) tensors of the same size")
        B = pred_rgb.numel() // (h * w * 3)
        mb = 0
        if mask is not None:
            if mask.dtype not in (torch.int32, torch.uint8, torch.bool) or not mask.is_contiguous():
                raise EnerfError("mask must be a contiguous int32 / uint8 / bool tensor")
            if mask.numel() != B * h * w:
                raise EnerfError(f"{what}: mask has {mask.numel()} elements, the images {B * h * w} pixels")
            mb = mask.element_size()
        if rect is not None:
            mode, abcd = RECT_XYWH, tuple(int(v) for v in rect)
            if len(abcd) != 4:
                raise EnerfError(f"{what}: rect must be (x, y, w, h)")
        elif (int(crop[0]), int(crop[1])) != (0, 0):
            mode, abcd = RECT_CROP, (int(crop[0]), int(crop[1]), 0, 0)
        else:
            mode, abcd = RECT_NONE, (0, 0, 0, 0)
        return h, w, B, mb, mode, abcd

    def eval_lpips(self, packed, pred_rgb, gt_rgb, mask=None, image_hw=None, crop=(0, 0), rect=None, mask_is_one=False, sync=True):
        """``loss_fn_vgg(pred, gt)`` of evaluators/enerf.py:81-87 / enerf_human.py:71-77 (lpips.LPIPS(net='vgg')) on device, with the
        evaluators' preprocessing: pixels whose ``mask`` is off (``>= 1`` is on; ``== 1`` with ``mask_is_one``) count as 0, the
        image is the ``eval_center`` slice ``crop`` = (crop_h, crop_w) or the rectangle ``rect`` = (x, y, w, h) (host values: for the
        human evaluator, ``mask_bbox`` read back), then (x - 0.5) * 2.  ``packed``: ``lpips_pack``'s image (the weights are the
        caller's).  ``pred_rgb`` / ``gt_rgb``: (B, h*w, 3) or (h*w, 3) with ``image_hw`` = (h, w).  Returns one float per image after
        ONE 48*B-byte D2H copy — or, with ``sync=False``, the (B,6) float64 device tensor {lpips, d_0 .. d_4}; nothing synchronises
        then.  A rectangle under 16 pixels in either extent, or outside the image, raises."""
        h, w, B, mb, mode, abcd = self._lpips_args("eval_lpips", pred_rgb, gt_rgb, mask, image_hw, crop, rect)
        pp, gp, kp = _ptr(pred_rgb), _ptr(gt_rgb), _ptr(packed)
        nbytes = self.dll.enerf_eval_lpips_workspace_bytes(B, h, w, mode, *abcd)
        if nbytes == 0:
            raise EnerfError(f"eval_lpips failed: {self.dll.enerf_last_error().decode()}")
        ws = torch.empty(((nbytes + 7) // 8,), dtype=torch.float64, device=pred_rgb.device)
        out = torch.empty((B, 6), dtype=torch.float64, device=pred_rgb.device)
        self._check(self.dll.enerf_eval_lpips(kp, pp, gp, None if mask is None else mask.data_ptr(), mb, int(bool(mask_is_one)), B, h, w,
                                              mode, *abcd, ws.data_ptr(), nbytes, out.data_ptr(), self.stream_of(pred_rgb)), "eval_lpips")
        if not sync:
            return out
        return out.cpu()[:, 0].tolist()

    def lpips_front(self, packed, pred_rgb, gt_rgb, mask=None, image_hw=None, crop=(0, 0), rect=None, mask_is_one=False):
        """The first layer of ``eval_lpips`` alone (preprocessing, scaling layer, conv 0 + ReLU): (2B, rh, rw, 64) channels-last,
        the pred images first, then the gt images."""
        h, w, B, mb, mode, abcd = self._lpips_args("lpips_front", pred_rgb, gt_rgb, mask, image_hw, crop, rect)
        rh, rw = (abcd[3], abcd[2]) if mode == RECT_XYWH else (h - 2 * abcd[0], w - 2 * abcd[1])
        out = torch.empty((2 * B, max(rh, 1), max(rw, 1), 64), dtype=torch.float32, device=pred_rgb.device)
        self._check(self.dll.enerf_lpips_front(_ptr(packed), _ptr(pred_rgb), _ptr(gt_rgb), None if mask is None else mask.data_ptr(), mb,
                                               int(bool(mask_is_one)), B, h, w, mode, *abcd, _ptr(out), self.stream_of(pred_rgb)),
                    "lpips_front")
        return out

    def vgg_conv3x3_pack(self, w, b):
        """w (cout,cin,3,3), b (cout) of one VGG16 layer -> its packed image (A operands | bias)."""
        cout, cin = int(w.shape[0]), int(w.shape[1])
        n = self.dll.enerf_vgg_conv3x3_packed_floats(cin, cout)
        if n == 0 or tuple(w.shape[2:]) != (3, 3) or tuple(b.shape) != (cout,):
            raise EnerfError(f"vgg_conv3x3_pack: unsupported layer {tuple(w.shape)} + {tuple(b.shape)} (not a VGG16 3x3 pair)")
        packed = torch.empty((n,), dtype=torch.float32, device=w.device)
        self._check(self.dll.enerf_vgg_conv3x3_pack(_ptr(w), _ptr(b), cin, cout, _ptr(packed), self.stream_of(w)), "vgg_conv3x3_pack")
        return packed

    def vgg_conv3x3(self, packed_layer, cin, cout, x_cl, relu=True):
        """One trunk layer on a channels-last tensor: x_cl (N,H,W,cin) -> (N,H,W,cout); 3x3, stride 1, zero padding 1, bias, ReLU."""
        if x_cl.dim() != 4 or x_cl.shape[3] != cin:
            raise EnerfError(f"vgg_conv3x3: input must be (N,H,W,{cin}) channels-last, got {tuple(x_cl.shape)}")
        N, H, W, _ = x_cl.shape
        out = torch.empty((N, H, W, cout), dtype=torch.float32, device=x_cl.device)
        self._check(self.dll.enerf_vgg_conv3x3(_ptr(packed_layer), int(cin), int(cout), _ptr(x_cl), _ptr(out), N, H, W, int(bool(relu)),
                                               self.stream_of(x_cl)), "vgg_conv3x3")
        return out

    # -- trainer's perceptual term (csrc/perceptual_vgg.h) ---------------------------------------------
    def perceptual_pack(self, convs):
        """``convs``: ten (w (cout,cin,3,3), b (cout)) pairs of VGG16 ``features[:23]`` in trunk order -> the packed image
        ``perceptual_fwd`` / ``perceptual_bwd`` read (``enerf_amd.loss.PerceptualWeights`` builds the list)."""
        if len(convs) != 10:
            raise EnerfError("perceptual_pack needs 10 (w, b) pairs")
        raw = PerceptualRaw()
        for i, ((w, b), (cin, cout)) in enumerate(zip(convs, PERCEPTUAL_CONVS)):
            if tuple(w.shape) != (cout, cin, 3, 3) or tuple(b.shape) != (cout,):
                raise EnerfError(f"perceptual_pack: conv {i} must be ({cout},{cin},3,3) + ({cout},), got {tuple(w.shape)} + {tuple(b.shape)}")
            raw.conv[i].w, raw.conv[i].b = _ptr(w), _ptr(b)
        packed = torch.empty((self.dll.enerf_perceptual_packed_floats(),), dtype=torch.float32, device=convs[0][0].device)
        self._check(self.dll.enerf_perceptual_pack(C.byref(raw), _ptr(packed), self.stream_of(packed)), "perceptual_pack")
        return packed

    def perceptual_workspace(self, N, h, w, device):
        """A workspace for N image pairs of h x w (float32 tensor; its byte size is what the C entries are told)."""
        nbytes = self.dll.enerf_perceptual_workspace_bytes(int(N), int(h), int(w))
        if nbytes == 0:
            raise EnerfError(f"perceptual loss failed: {self.dll.enerf_last_error().decode()}")
        return torch.empty((nbytes // 4,), dtype=torch.float32, device=device)

    def perceptual_layout(self, N, h, w):
        """[(float offset, (2N, H_i, W_i, C_i))] of the ten saved activations in the workspace: pred images first, then gt."""
        offs = (_ll * 10)()
        self._check(self.dll.enerf_perceptual_layout(int(N), int(h), int(w), offs), "perceptual_layout")
        out, H, W = [], int(h), int(w)
        for i, (_, cout) in enumerate(PERCEPTUAL_CONVS):
            if i in (2, 4, 7):
                H, W = H // 2, W // 2
            out.append((int(offs[i]), (2 * int(N), H, W, cout)))
        return out

    def perceptual_fwd(self, packed, pred_rgb, gt_rgb, image_hw, workspace=None):
        """pred / gt (N, h*w, 3) -> (out, workspace): out 5 float64 on the device {loss, l_0 .. l_3} (no host read), the workspace
        holding the ten saved activations ``perceptual_bwd`` needs."""
        h, w = int(image_hw[0]), int(image_hw[1])
        if h <= 0 or w <= 0 or pred_rgb.numel() == 0 or pred_rgb.numel() % (h * w * 3) or gt_rgb.numel() != pred_rgb.numel():
            raise EnerfError(f"perceptual_fwd: pred / gt must be (N, {h}*{w}, 3) tensors of the same size")
        N = pred_rgb.numel() // (h * w * 3)
        ws = workspace if workspace is not None else self.perceptual_workspace(N, h, w, pred_rgb.device)
        out = torch.empty((5,), dtype=torch.float64, device=pred_rgb.device)
        self._check(self.dll.enerf_perceptual_fwd(_ptr(packed), _ptr(pred_rgb), _ptr(gt_rgb), N, h, w, ws.data_ptr(), ws.numel() * 4,
                                                  out.data_ptr(), self.stream_of(pred_rgb)), "perceptual_fwd")
        return out, ws

    def perceptual_bwd(self, packed, N, image_hw, workspace, grad_scale=None):
        """d loss / d pred (N, h*w, 3) from the workspace ``perceptual_fwd`` left; ``grad_scale``: a float32 device scalar or None."""
        h, w = int(image_hw[0]), int(image_hw[1])
        if grad_scale is not None and grad_scale.numel() != 1:
            raise EnerfError("perceptual_bwd: grad_scale must hold one float")
        grad = torch.empty((int(N), h * w, 3), dtype=torch.float32, device=workspace.device)
        self._check(self.dll.enerf_perceptual_bwd(_ptr(packed), int(N), h, w, workspace.data_ptr(), workspace.numel() * 4,
                                                  _ptr(grad_scale), _ptr(grad), self.stream_of(workspace)), "perceptual_bwd")
        return grad

    def vgg_conv3x3_dgrad_pack(self, w):
        """w (cout,cin,3,3) of one of the ten trunk layers -> the packed image of its data gradient."""
        cout, cin = int(w.shape[0]), int(w.shape[1])
        n = self.dll.enerf_vgg_conv3x3_dgrad_packed_floats(cin, cout)
        if n == 0 or tuple(w.shape[2:]) != (3, 3):
            raise EnerfError(f"vgg_conv3x3_dgrad_pack: unsupported layer {tuple(w.shape)} (not one of the ten trunk layers)")
        packed = torch.empty((n,), dtype=torch.float32, device=w.device)
        self._check(self.dll.enerf_vgg_conv3x3_dgrad_pack(_ptr(w), cin, cout, _ptr(packed), self.stream_of(w)), "vgg_conv3x3_dgrad_pack")
        return packed

    def vgg_conv3x3_dgrad(self, packed, cin, cout, gout_cl):
        """The gradient of one trunk layer (cin -> cout) with respect to its input, plain: gout_cl (N,H,W,cout) -> (N,H,W,cin)."""
        if gout_cl.dim() != 4 or gout_cl.shape[3] != cout:
            raise EnerfError(f"vgg_conv3x3_dgrad: gradient must be (N,H,W,{cout}) channels-last, got {tuple(gout_cl.shape)}")
        N, H, W, _ = gout_cl.shape
        out = torch.empty((N, H, W, cin), dtype=torch.float32, device=gout_cl.device)
        self._check(self.dll.enerf_vgg_conv3x3_dgrad(_ptr(packed), int(cin), int(cout), _ptr(gout_cl), _ptr(out), N, H, W,
                                                     self.stream_of(gout_cl)), "vgg_conv3x3_dgrad")
        return out

    def mask_bbox(self, mask, image_hw, mask_is_one=False, sync=True):
        """cv2.boundingRect of the on pixels (enerf_human.py:64) per image: mask (B, h*w) -> (B,4) int32 {x, y, w, h} (all 0: nothing
        on).  ``sync=True`` returns a list of tuples after a 16*B-byte D2H copy; ``sync=False`` the device tensor."""
        h, w = int(image_hw[0]), int(image_hw[1])
        if mask.dtype not in (torch.int32, torch.uint8, torch.bool) or not mask.is_contiguous() or mask.numel() % (h * w):
            raise EnerfError("mask must be a contiguous int32 / uint8 / bool tensor of B*h*w elements")
        B = mask.numel() // (h * w)
        rect = torch.empty((B, 4), dtype=torch.int32, device=mask.device)
        self._check(self.dll.enerf_mask_bbox(mask.data_ptr(), mask.element_size(), int(bool(mask_is_one)), B, h, w, rect.data_ptr(),
                                             self.stream_of(mask)), "mask_bbox")
        if not sync:
            return rect
        return [tuple(r) for r in rect.cpu().tolist()]

    def depth_stats(self, pred_depth, gt_depth, sync=True):
        """The depth statistics alone (evaluators/enerf.py:96-103: abs / acc_2 / acc_10 over gt != 0): enerf_eval_stats with
        no rgb.  Returns dict(abs, acc_2, acc_10) — empty when no pixel has ground truth."""
        acc = torch.empty((6,), dtype=torch.float64, device=pred_depth.device)
        self._check(self.dll.enerf_eval_stats(None, None, None, 0, 0, 0, 0, 0, 0, _ptr(pred_depth), _ptr(gt_depth),
                                              pred_depth.numel(), acc.data_ptr(), self.stream_of(pred_depth)), "eval_stats")
        if not sync:
            return acc
        a = acc.cpu().tolist()
        return dict(abs=a[2] / a[3], acc_2=a[4] / a[3], acc_10=a[5] / a[3]) if a[3] > 0 else {}


def stats_from_acc(a) -> dict:
    import math
    out = {"psnr": 10.0 * math.log10(a[1] / a[0]) if a[0] > 0 else float("inf")}
    if a[3] > 0:
        out.update(abs=a[2] / a[3], acc_2=a[4] / a[3], acc_10=a[5] / a[3])
    return out


_LIB: Optional[EnerfLib] = None


def get_lib() -> EnerfLib:
    """The product library (HIP, gfx950).  Raises if it has not been built — never falls back."""
    global _LIB
    if _LIB is None:
        _LIB = EnerfLib(LIB_PATH)
    return _LIB
