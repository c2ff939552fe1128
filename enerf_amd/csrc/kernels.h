// kernels.h — host-side launchers implemented by the .hip files in this directory.
// All pointers are device pointers; nothing here allocates or synchronises.
#pragma once
#include "common.h"
#include "../../include/enerf_hip.h"

namespace enerf {

// Explicit kernel-variant choices (include/enerf_hip.h: enerf_options_t); a NULL pointer at the C ABI means all zero.
using Options = enerf_options_t;
inline Options resolve_options(const enerf_options_t* o) { return o ? *o : Options{}; }
// error reporting shared by the C-ABI translation units (capi.hip, frame.hip): thread-local message + code
int fail(int code, const char* fmt, ...);
int check_launch(const char* what);
const char* last_error();
#define REQUIRE(cond, ...) \
    do { if (!(cond)) return ::enerf::fail(ENERF_EINVAL, __VA_ARGS__); } while (0)
// number of compute units of the current device (queried once per device; 256 on MI355X)
int device_cu_count();
// Zero `bytes` (a multiple of 4) on the stream with a fill KERNEL: a hipMemsetAsync becomes a memset node when the stream is
// being captured, and those did not replay reliably inside a whole-training-step hipGraph on this stack.
void zero_async(void* p, size_t bytes, hipStream_t st);
void zero_async2(void* p, size_t bytes_p, void* q, size_t bytes_q, hipStream_t st);

// ---- geometry.hip -------------------------------------------------------------------------------
void launch_channels_last(const float* src, float* dst, int n, int C, long long P, int Cpad, hipStream_t st);
void launch_channels_first(const float* src, float* dst, int n, int C, long long P, int Cpad, hipStream_t st);
void launch_pack_img_feat_rgb(const float* im_feat, int C, int Hf, int Wf, const float* src_inps, int H, int W,
                              int Hr, int Wr, int tex, int n_img, float* out, hipStream_t st);
void launch_proj_mats(const float* src_ixts, const float* src_exts, const float* tar_ixt, const float* tar_ext, int B,
                      int S, float src_scale, float tar_scale, float* proj, hipStream_t st);
void launch_depth_values(const float* near_far, const float* pdepth, const float* pstd, const float* pnf, int B, int D,
                         int h, int w, int hp, int wp, int depth_inv, float* dv, float* nf_out, hipStream_t st);
void launch_level_prep(const float* src_ixts, const float* src_exts, const float* tar_ixt, const float* tar_ext, int S,
                       float src_scale, float tar_scale, float* proj, const float* near_far, const float* pdepth,
                       const float* pstd, const float* pnf, int B, int D, int h, int w, int hp, int wp, int depth_inv,
                       float* dv, float* nf_out, hipStream_t st);     // proj_mats + depth_values in one launch
// depth_mvs (optional): 1/depth for disparity-space levels, depth otherwise (network.py:105-108)
void launch_depth_regression(const float* prob, const float* dv, int B, int D, int h, int w, int depth_inv,
                             float* depth, float* std, float* depth_mvs, hipStream_t st);
// depth_regression of the previous (not rendered) level + proj_mats + depth_values of this level in one launch; false = shape
// not handled, nothing launched
bool launch_regress_and_values(const float* src_ixts, const float* src_exts, const float* tar_ixt, const float* tar_ext, int S,
                               float src_scale, float tar_scale, float* proj, const float* prob_p, const float* dv_p,
                               const float* nf_p, int Dp, int hp, int wp, int depth_inv_p, float* depth_p, float* std_p, int B,
                               int D, int h, int w, int depth_inv, float* dv, float* nf_out, hipStream_t st);
void launch_build_rays(const float* rays8, const float* depth, const float* std, const float* nf, int B, int N, int h,
                       int w, int Hr, int Wr, int depth_inv, float* rays12, hipStream_t st);

// ---- volume.hip ---------------------------------------------------------------------------------
// planar = 1: vol as channel-quad planes (B, C/4, D, h, w, 4) instead of channels-last (B, D, h, w, C)
void launch_feature_volume(const float* feat_nhwc, const float* proj, const float* dv, int B, int S, int C, int Hs,
                           int Ws, int D, int h, int w, float* vol, hipStream_t st, int planar = 0);
// does conv0 of this cost-reg network read the volume as channel-quad planes? (the frame driver asks before the warp: the answer is
// conv0's route in the plan cost_reg_run itself launches from, capi.hip cost_reg_plan)
bool cost_reg_conv0_planar(const enerf_options_t& o, int in_channels, int full, int B, int D, int h, int w);
// may this cost-reg network run without its feature output (cost_reg_run with feat == nullptr)?  True when the fused heads' route in
// the same plan is a kernel that skips the feature channels on a null pointer (conv3d_route_optional_out)
bool cost_reg_feat_optional(const enerf_options_t& o, int in_channels, int full, int B, int D, int h, int w);
// enerf_cost_reg with the volume layout made explicit (vol_planar = 1: channel-quad planes, see launch_feature_volume)
// feat == nullptr: prob only — the heads skip the eight feature channels nobody will read (needs cost_reg_feat_optional)
// hook: called on the host right after layer `after_layer` (0 = conv0) has been enqueued (enerf_forward uses it to start a
// side-lane stage at that point of the chain); nullptr = none
struct CostRegHook { void (*fn)(void* ctx); void* ctx; int after_layer; };
int cost_reg_run(const float* packed, int in_channels, int full, const float* vol, int vol_planar, int B, int D, int h, int w,
                 float* feat, float* prob, void* workspace, size_t workspace_bytes, const enerf_options_t* options, hipStream_t st,
                 const CostRegHook* hook = nullptr);

// ---- conv3d.hip ---------------------------------------------------------------------------------
enum ConvKind { kConvS1 = 0, kConvS2 = 1, kConvT2 = 2 };
struct Conv3dDesc {
    const float* w;         // packed A operands (see conv3d.hip)
    const float* scale;     // per-cout epilogue scale (BN folded; 1 without BN), padded to 16*row tiles
    const float* shift;     // per-cout epilogue shift (0 without BN)
    int cin, cout, kind, relu;
    const float* w_pk8;     // tap-packed image for stride-1 cout=8(+1) layers (conv3d_pk8.hip) or nullptr
    const float* w_b4;      // batched-4x4 image for the same layers (conv3d_b4.hip) or nullptr
    const float* w_t2pair;  // x-parity-paired image of a transposed 16 -> 8 layer (conv3d_t2.hip) or nullptr
    int in_planar;          // input is channel-quad planes (B, cin/4, D, H, W, 4): only the glds b4 kernel reads that
    int out_planar;         // output as channel-quad planes: only the class-paired transposed kernel writes that
};
long long conv3d_t2_pair_floats();
void launch_conv3d_t2_pair_pack(const float* packed, float* paired, hipStream_t st);   // from the class-major packed image
long long conv3d_b4_packed_floats(int cin);      // batched 4x4x1 image for cout = 8 (+ optional depth row on the VALU): conv3d_b4.hip
void launch_conv3d_b4_pack(const float* w, const float* wd, int cin, float* packed, hipStream_t st);
long long conv3d_pk8_packed_floats(int cin);     // tap-packed image for cout = 8 (+ optional depth row): conv3d_pk8.hip
void launch_conv3d_pk8_pack(const float* w, const float* wd, int cin, float* packed, hipStream_t st);

// Which kernel a layer runs.  conv3d_route decides it from values alone (no HIP call, no pointer, no static state); the launchers
// below take the route and only size the grid.  The fields are the template values of the instantiation, named as the kernels name
// them; conv3d_route_name prints them in the kernel's template order: s1_b4g<16,4,false>, conv3d<32,1,0,1,3>, wl<32,0,2>.
enum Conv3dFamily {
    kRouteNone = 0,      // no kernel handles the layer shape
    kRouteT2All,         // k_conv3d_t2_all<cin, cout, 1, 4>: every-class transposed kernel; cout = 8 is the x-parity-paired form
    kRouteT2Lds,         // k_conv3d_t2_lds<16>
    kRouteS2Lds,         // k_conv3d_s2_lds<8>
    kRouteB4,            // k_conv3d_s1_b4<cin, bd, heads>: register-staged batched 4x4
    kRouteB4g,           // k_conv3d_s1_b4g<cin, 4, heads>: asynchronously staged (reads channels-last or channel-quad planes)
    kRouteB4c,           // k_conv3d_s1_b4c<cin, 4, heads>: the same with register-held weights, four blocks per CU
    kRoutePk8,           // k_conv3d_s1_pk8<cin, bd>
    kRouteS1Lds,         // k_conv3d_s1_lds<cin, rt, bd, bh>
    kRouteWl,            // k_conv3d_wl<cin, kind, ctb> over kd taps kdlo .. kdlo + nkd - 1
    kRouteGlobal         // k_conv3d<cin, rt, kind, ct, split>
};
struct Conv3dRoute {
    int family = kRouteNone;
    int cin = 0, cout = 0, kind = 0;
    int bd = 0, bh = 0;                 // output box depth / height of the LDS-staged stride-1 families
    bool heads = false;                 // b4 families: the fused feat ++ depth heads (depth row on the VALU)
    int rt = 0, ct = 0, split = 0;      // k_conv3d: row tiles and column tiles per wave, kd split; rt also k_conv3d_s1_lds's
    int ctb = 0, kdlo = 0, nkd = 0;     // k_conv3d_wl: column tiles per block, the kd taps that fall inside the volume.  (A wl route keeps
                                        // the layer's k_conv3d values in rt / ct / split: launch_conv3d's one fallback.)
};
// what the route needs to know of a layer: its shape and which extra weight images were packed for it
struct Conv3dLayer { int cin, cout, kind; bool pk8, b4, t2pair; };
Conv3dRoute conv3d_route(const Conv3dLayer& L, bool has_residual, bool has_out2, int B, int Di, int Hi, int Wi, const Options& o,
                         int cu_count);
bool conv3d_route_planar_in(const Conv3dRoute& r);      // the kernel can read channel-quad planes (b4g / b4c)
bool conv3d_route_planar_out(const Conv3dRoute& r);     // the kernel can write them (the paired t2_all)
bool conv3d_route_optional_out(const Conv3dRoute& r);   // fused heads whose kernel takes out == nullptr: depth head only (b4 families)
void conv3d_route_name(const Conv3dRoute& r, char* buf, size_t cap);

// The per-file launchers: geometry only, the route has decided.
void launch_conv3d_b4(const Conv3dDesc& L, const Conv3dRoute& r, const float* in, float* out, float* out2, int B, int D, int H, int W,
                      hipStream_t st);
void launch_conv3d_pk8(const Conv3dDesc& L, const Conv3dRoute& r, const float* in, float* out, float* out2, int B, int D, int H, int W,
                       hipStream_t st);
void launch_conv3d_s2_lds(const Conv3dDesc& L, const float* in, float* out, int B, int Di, int Hi, int Wi, hipStream_t st);
void launch_conv3d_t2_lds(const Conv3dDesc& L, const float* in, const float* residual, float* out, int B, int Di, int Hi, int Wi,
                          hipStream_t st);
void launch_conv3d_t2_all(const Conv3dDesc& L, const Conv3dRoute& r, const float* in, const float* residual, float* out, int B, int Di,
                          int Hi, int Wi, hipStream_t st);
// false: the runtime refused the > 64 KB dynamic LDS opt-in this instantiation needs; nothing launched (see launch_conv3d)
bool launch_conv3d_wl(const Conv3dDesc& L, const Conv3dRoute& r, const float* in, float* out, int B, int Di, int Hi, int Wi,
                      hipStream_t st);
// number of floats of the packed weight image for a layer
long long conv3d_packed_floats(int cin, int cout, int kind);
// pack torch-layout weights (Conv3d: (cout,cin,3,3,3); ConvTranspose3d: (cin,cout,3,3,3)) + BN into
// {packed A operands, scale[coutpad], shift[coutpad]}
// rows [0,cout1) of the GEMM come from w, rows [cout1,cout) from w2 (used to fuse feat_conv ++ depth_conv)
void launch_conv3d_pack(const float* w, const float* w2, int cout1, const float* bn_w, const float* bn_b, const float* bn_mean, const float* bn_var,
                        float eps, int cin, int cout, int kind, float* packed, float* scale, float* shift,
                        hipStream_t st);
// One layer's packed image: [weights | scale | shift | pk8 image | b4 image] or [weights | scale | shift | t2-pair image], offsets in
// floats, -1 = the layer has no such image.  cout8_images: the stride-1 cout = 8 (+ 1) layers of the cost-reg nets (conv0, fused heads).
struct Conv3dImage { long long w, scale, shift, pk8, b4, t2pair, floats; };
inline Conv3dImage conv3d_layer_image(int cin, int cout, int kind, bool cout8_images) {
    Conv3dImage im = {0, conv3d_packed_floats(cin, cout, kind), 0, -1, -1, -1, 0};
    im.shift = im.scale + cdiv(cout, 16) * 16;
    im.floats = im.shift + cdiv(cout, 16) * 16;
    if (cout8_images) {
        im.pk8 = im.floats;
        im.b4 = im.pk8 + conv3d_pk8_packed_floats(cin);
        im.floats = im.b4 + conv3d_b4_packed_floats(cin);
    }
    if (kind == kConvT2 && cin == 16 && cout == 8) {        // conv11: x-parity-paired A operands
        im.t2pair = im.floats;
        im.floats += conv3d_t2_pair_floats();
    }
    return im;
}
inline Conv3dLayer conv3d_layer_of(const Conv3dImage& im, int cin, int cout, int kind) {
    return {cin, cout, kind, im.pk8 >= 0, im.b4 >= 0, im.t2pair >= 0};
}
inline Conv3dDesc conv3d_desc(const float* p, const Conv3dImage& im, int cin, int cout, int kind, int relu) {
    return {p + im.w, p + im.scale, p + im.shift, cin, cout, kind, relu, im.pk8 >= 0 ? p + im.pk8 : nullptr,
            im.b4 >= 0 ? p + im.b4 : nullptr, im.t2pair >= 0 ? p + im.t2pair : nullptr, 0, 0};
}
// in: (B, Di, Hi, Wi, cin) channels-last; out: (B, Do, Ho, Wo, cout_store); residual (same shape as out) optional.
// cout_store lets the fused heads write feat (8 ch) and prob (1 ch) to two tensors: if out2 != nullptr,
// channels [0,8) go to out (stride 8) and channel 8 goes to out2 (stride 1).
// r = conv3d_route(...) of this layer with these operands.  Returns false for kRouteNone (nothing launched).
bool launch_conv3d(const Conv3dDesc& L, const Conv3dRoute& r, const float* in, const float* residual, float* out, float* out2, int B,
                   int Di, int Hi, int Wi, hipStream_t st);

// ---- wgrad.hip ----------------------------------------------------------------------------------
// One weight gradient dW[a][b][taps] = sum over the positions of the A grid (include/enerf_hip.h: enerf_conv_wgrad; enerf_gemm_wgrad
// is the 1x1x1 problem on a 1 x 1 x P grid with row strides).
struct WgradShape {
    int n, Da, Ha, Wa, Ca;      // A grid (the positions summed over) and channels
    int Db, Hb, Wb, Cb;         // B grid and channels
    int lda, ldb;               // floats between consecutive positions of A / B (>= Ca / Cb)
    int kd, kh, kw, stride, pad_d, pad_h, pad_w;
    int bias;                   // 1: also dbias[a] = sum over the positions of A[a] (a virtual all-ones column Cb of B)
    bool linear;                // enerf_gemm_wgrad's problem: k_gemm_wgrad whenever its tiles fit, in every A/B build
};
// Which kernel a weight gradient runs, as conv3d_route above: wgrad_route decides from values alone (no HIP call, no pointer, no static
// state), the launcher in wgrad.hip launches what it decided, second stage included.  The upper-case fields are the template values of
// the instantiation under the kernels' own names; wgrad_route_name prints them in template order: wgrad2d_3x3_p16<1,2>,
// conv_wgrad<3,3,3,3,2>, gemm_wgrad<2,3>.
enum WgradFamily {
    kWgradNone = 0,     // no kernel handles the kernel extents
    kWgradGemm,         // k_gemm_wgrad<TA, TB>: 1x1x1 stride 1, <= 4 x 6 channel tiles; second stage k_wgrad_reduce
    kWgrad2dC8,         // k_wgrad2d_3x3_c8<A4, B4, NCB>: 1x3x3 stride 1, <= 8 A channels; second stage k_colsum
    kWgrad2dP16,        // k_wgrad2d_3x3_p16<NA, NB>: ... 16 / 32 channels on both sides; k_colsum
    kWgrad3dC8,         // k_wgrad3d_c8<A4, NCB>: 3x3x3 stride 1, <= 8 channels on one side (swapped: on the B side); k_colsum
    kWgradGeneric       // k_conv_wgrad<KD, KH, KW, SPLIT, PL>: everything else; k_wgrad_reduce
};
struct WgradRoute {
    int family = kWgradNone;
    int TA = 0, TB = 0;                                 // k_gemm_wgrad
    bool A4 = false, B4 = false;                        // c8 kernels: 16-byte (true) or scalar staging of the A / B tile
    int NCB = 0, NA = 0, NB = 0;                        // c8: blocks of 8 B channels per launch column; p16: 16-channel blocks of A / B
    bool swapped = false;                               // k_wgrad3d_c8: the kernel's A is the caller's B (the <= 8-channel side)
    int KD = 0, KH = 0, KW = 0, SPLIT = 0, PL = 0;      // k_conv_wgrad
    int blocks = 0, cols = 1;                           // first stage's grid (x, y); y = 2: the two halves of a 32-channel B (3-D)
    int chunks = 0;                                     // partial results per output element: what the second stage sums
    int tiles_a = 0, tiles_b = 0;                       // gemm / generic: 16-channel tiles of A and of B (+ bias column)
    int tiles_y = 0, tiles_x = 0;                       // tile kernels: image tiles per plane
    size_t scratch_bytes = 0;                           // bytes of the caller's workspace the two stages use
    bool atomic = false;                                // gemm / generic with a workspace below their two-stage form: no second stage,
                                                        // fp32 atomics onto a grad_w (and grad_bias) the caller zeroes first
};
// a16 / b16: the A / B base address is 16-byte aligned.  workspace_bytes: 0 without a workspace.
WgradRoute wgrad_route(const WgradShape& p, bool a16, bool b16, size_t workspace_bytes, int cu_count);
void wgrad_route_name(const WgradRoute& r, char* buf, size_t cap);
const char* wgrad_route_second_stage(const WgradRoute& r);     // "wgrad_reduce", "colsum" or "" (atomic commit)

// ---- conv2d.hip (FeatureNet) ----------------------------------------------------------------------
struct Conv2dDesc {
    const float* w;        // packed A operands
    const float* scale;    // per-cout scale (BN folded; 1 for plain convs)
    const float* shift;    // per-cout shift (BN folded, or the conv bias)
    int cin, cout, k, stride, relu;
    int out_stride;        // floats between consecutive output pixels (0 = cout)
    const float* rgb_src;  // texel mode: (n,3,Ho,Wo) images appended as [rgb*0.5+0.5 | 0] behind the features
    const float* chain_w;      // packed weights / shift (bias) of a following 1x1 conv (cout -> 32) applied in the
    const float* chain_shift;  // epilogue instead of storing this layer's output (conv2.1 -> toplayer), or nullptr
};
long long conv2d_packed_floats(int cin, int cout, int k);
void launch_conv2d_pack(const float* w, const float* bias, const float* bn_w, const float* bn_b, const float* bn_mean,
                        const float* bn_var, float eps, int cin, int cout, int k, float* packed, float* scale,
                        float* shift, hipStream_t st);
// in: channels-last (N,Hi,Wi,cin) — or the NCHW image batch for the 3-channel first layer; out: channels-last.
// up (optional): coarser channels-last map (N,Hc,Wc,cout) added after a x2 align-corners bilinear upsample.
int launch_conv2d(const Conv2dDesc& L, const float* in, float* out, const float* up, int N, int Hi, int Wi, int Hc,
                  int Wc, hipStream_t st);
// conv0.1(conv0.0(image)) fused (feature_net.py:7-9): L0/L1 = the two layers' descriptors, img (N,3,H,W) -> out (N,H,W,8)
// job (prep_job.h, optional): the frame's camera-only preparation carried by extra blocks of this launch; returns whether it was
struct PrepJob;
bool launch_conv0_fused(const Conv2dDesc& L0, const Conv2dDesc& L1, const float* w_cb0, const float* w_cb1, const float* img,
                        float* out, int N, int H, int W, hipStream_t st, const PrepJob* job = nullptr);
// enerf_feature_net_stage with a preparation job for the trunk's first launch; *job_done = 1 when a kernel carried it
int feature_net_stage_job(const float* packed, const float* src_inps, int n_img, int H, int W, float* feat_l0, float* feat_l1,
                          float* feat_l2, int l2_stride, void* workspace, size_t workspace_bytes, int stage,
                          const enerf_options_t* options, hipStream_t stream, const PrepJob* job, int* job_done);
// smooth0(up2(f1pre) + lat0(c0)) fused (feature_net.py:32-35); L = smooth0's descriptor, lat_w/lat_b raw (32,8)/(32)
// smooth1(up2(f2) + lat1(c1)) fused (feature_net.py:33-34, round 5): writes f1pre (N,H1,W1,32) and out (N,H1,W1,16); false: not applicable
bool launch_smooth1_fused(const Conv2dDesc& Llat, const Conv2dDesc& Lsm, const float* c1, const float* f2, float* f1pre, float* out,
                          int N, int H1, int W1, hipStream_t st);
// w_cb: the layer's broadcast-A image (launch_conv2d_cb_pack)
void launch_smooth0_fused(const Conv2dDesc& L, const float* c0, const float* f1pre, const float* lat_w, const float* lat_b,
                          const float* w_cb, float* out, int N, int H, int W, hipStream_t st);
// broadcast-A image (common.h mfma4_bc) of input channels ci0 .. ci0+cinp-1 of a 3x3, Cout = 8 layer: ceil(18*cinp/16)*64 floats
void launch_conv2d_cb_pack(const float* w, int cin, int ci0, int cinp, float* packed, hipStream_t st);
// texels from channels-last features at the render resolution + resized colours (general case)
void launch_pack_texels_cl(const float* feat_cl, int C, const float* src_inps, int H, int W, int Hr, int Wr, int tex,
                           int n_img, float* out, hipStream_t st);

// ---- io.hip (the steps before/after the path: SURVEY.md 8f rows 3,4) --------------------------------
void launch_gen_rays(const float* tar_ext, const float* tar_ixt, int B, int Hr, int Wr, float scale, float* rays,
                     hipStream_t st);
void launch_pack_rgb8(const float* rgb, int H, int W, int flip, unsigned char* out, hipStream_t st);
void launch_eval_stats(const float* pred_rgb, const float* gt_rgb, const void* mask, int mask_bytes, long long n_rgb,
                       int img_w, int img_h, int crop_h, int crop_w, const float* pred_depth, const float* gt_depth,
                       long long n_depth, double* acc, hipStream_t st);
// SSIM of the evaluators (skimage's structural_similarity on the cropped / boxed, mask-zeroed images); workspace: boxes | partials
size_t eval_ssim_workspace_bytes(int B, int img_h, int img_w, int rect_mode, int crop_h, int crop_w);
void launch_eval_ssim(const float* pred_rgb, const float* gt_rgb, const void* mask, int mask_bytes, int mask_mode, int B,
                      int img_h, int img_w, int rect_mode, int crop_h, int crop_w, void* workspace, double* out,
                      hipStream_t st);
// LPIPS of the evaluators (lpips_vgg.h, included by io.hip): the VGG16 trunk as 3x3 fp32-MFMA convolutions + the five taps.
// pool: a 2x2 / stride 2 / floor max pool in front of the layer; tap: the tap taken after it, or -1
struct VggLayerSpec { int cin, cout, pool, tap; };
constexpr int kVggLayers = 13;
constexpr VggLayerSpec kVggSpec[kVggLayers] = {{3, 64, 0, -1},   {64, 64, 0, 0},    {64, 128, 1, -1},  {128, 128, 0, 1}, {128, 256, 1, -1},
                                               {256, 256, 0, -1}, {256, 256, 0, 2},  {256, 512, 1, -1}, {512, 512, 0, -1}, {512, 512, 0, 3},
                                               {512, 512, 1, -1}, {512, 512, 0, -1}, {512, 512, 0, 4}};
constexpr int kLpipsTapC[5] = {64, 128, 256, 512, 512};
// conv 0 reading the evaluator's images: pred / gt (B, img_h*img_w, 3), the mask as enerf_eval_ssim takes it, the rectangle's corner
struct VggFront { const float* pred; const float* gt; const unsigned char* mask; int mask_bytes, mask_mode, B, img_h, img_w, y0, x0; };
bool vgg_conv3x3_supported(int cin, int cout);
long long vgg_conv3x3_packed_floats(int cin, int cout);
void launch_vgg_conv3x3_pack(const float* w, const float* bias, int cin, int cout, float* packed, hipStream_t st);
void launch_vgg_conv3x3(const float* packed_layer, int cin, int cout, const float* in, float* out, int N, int H, int W, int pool,
                        int Hin, int Win, int relu, const VggFront* front, hipStream_t st);
long long lpips_packed_floats();
void launch_lpips_pack(const enerf_lpips_raw_t& raw, float* packed, hipStream_t st);
size_t eval_lpips_workspace_bytes(int B, int rh, int rw);
void launch_eval_lpips(const float* packed, const VggFront& front, int rh, int rw, void* workspace, double* out, hipStream_t st);
void launch_mask_bbox(const void* mask, int mask_bytes, int mask_mode, int B, int img_h, int img_w, int* rect, hipStream_t st);
// The trainer's perceptual term (perceptual_vgg.h, included by io.hip): the first ten trunk layers forward with every output kept,
// L1 taps, and the ten data-gradient layers back into the rendered image.  (cin, cout) always name the FORWARD layer.
long long perceptual_packed_floats();
void launch_perceptual_pack(const enerf_perceptual_raw_t& raw, float* packed, hipStream_t st);
size_t perceptual_workspace_bytes(int N, int h, int w);
void perceptual_layout(int N, int h, int w, long long* offsets);
void launch_perceptual_fwd(const float* packed, const float* pred, const float* gt, int N, int h, int w, void* workspace, double* out,
                           hipStream_t st);
void launch_perceptual_bwd(const float* packed, int N, int h, int w, void* workspace, const float* grad_scale, float* grad_pred,
                           hipStream_t st);
bool vgg_dgrad_supported(int cin, int cout);
long long vgg_dgrad_packed_floats(int cin, int cout);
void launch_vgg_dgrad_pack(const float* w, int cin, int cout, float* packed, hipStream_t st);
void launch_vgg_conv3x3_dgrad(const float* packed_d, int cin, int cout, const float* gout, float* gin, int N, int H, int W,
                              hipStream_t st);
void launch_gen_rays_at(const float* tar_ext, const float* tar_ixt, const int* xy, int B, int N, float scale, float* rays,
                        hipStream_t st);
void launch_rays_bbox_mask(const float* rays, const float* bounds, long long n, int* mask, hipStream_t st);
void launch_select_views(const float* cam_points, int V, const float* c2w, int k, int* idx, hipStream_t st);
void launch_gather_views(const float* inps, const float* exts, const float* ixts, const int* idx, int k, int H, int W,
                         float* src_inps, float* src_exts, float* src_ixts, hipStream_t st);
void ingest_raw_geometry(int Hraw, int Wraw, double input_ratio, int* Hs, int* Ws);
void launch_ingest_raw_u8(const unsigned char* img, const unsigned char* mask, const float* ixts, const float* dist, int V, int Hraw,
                          int Wraw, double input_ratio, int crop_y, int crop_x, int H, int W, int dilate, unsigned char* mask_scratch,
                          float* out, unsigned char* mask_out, hipStream_t st);
void launch_ingest_views_u8(const unsigned char* img, const unsigned char* mask, int dilate, int V, int H, int W, float* out,
                            hipStream_t st);
void launch_bounds_near_far(const float* vertices, int n, const float* tar_ext, int B, float near_min, float* near_far,
                            hipStream_t st);

// ---- frame.hip (mask_at_box compaction; the frame driver — FrameRun's stages, run_frame — and its side lane, side_lane.h, live there too) ----
size_t mask_compact_workspace_bytes(long long n);
void launch_mask_compact(const void* mask, int elem_bytes, long long n, int* index, int* count, void* workspace,
                         hipStream_t st);

// ---- render.hip ---------------------------------------------------------------------------------
using NerfRaw = enerf_nerf_raw_t;     // torch-layout parameter pointers of one NeRF (nerf.py:6-89)
long long nerf_packed_floats(int feat_ch_plus3);
void launch_nerf_pack(const NerfRaw& raw, int F, int viewdir_agg, float* packed, hipStream_t st);
using RenderArgs = enerf_render_args_t;
int launch_render_rays(const RenderArgs& a, hipStream_t st);  // returns 0, or <0 for unsupported shapes
// the RAW instantiations: a.rgb = (n, Ns, 4) samples [r, g, b, sigma], a.depth = (n, Ns) metric sample depths, a.vol may be NULL
int launch_render_rays_raw(const RenderArgs& a, hipStream_t st);
int render_rays_raw_check(const RenderArgs& a);                // its refusals alone: 0 or the launcher's code, nothing launched

// ---- the composite network (network_composite.py): volume.hip, composite_layers.h (included by geometry.hip) ----
void launch_feature_volume_window(const float* feat_nhwc, const float* proj, const float* dv, int B, int S, int C, int Hs, int Ws, int D,
                                  int h, int w, int x0, int y0, int ww, int wh, float* vol, hipStream_t st);
void launch_depth_regression_window(const float* prob, const float* dv, int B, int D, int h, int w, int x0, int y0, int ww, int wh,
                                    int depth_inv, float* depth, float* std, hipStream_t st);
void launch_window_ray_index(int x0, int y0, int ww, int wh, int Wr, int* index, int* count, hipStream_t st);
void launch_composite_layers(const enerf_composite_layers_t& a, hipStream_t st, const int* invalid = nullptr);
// enerf_composite_layers with the cached frame's device flag (nonzero: every output NaN; nullptr: the C entry itself)
int composite_layers_run(const enerf_composite_layers_t* a, const int* invalid, hipStream_t st);
// the backwards the composite network's training step adds (backward.hip: the windowed template values; composite_layers.h)
void launch_feature_volume_window_bwd(const float* feat, const float* proj, const float* dv, const float* gvol, int B, int S, int C,
                                      int Hs, int Ws, int D, int h, int w, int x0, int y0, int ww, int wh, float* gfeat, float* gdv,
                                      hipStream_t st);
void launch_depth_regression_window_bwd(const float* prob, const float* dv, const float* g_depth, const float* g_std, int B, int D,
                                        int h, int w, int x0, int y0, int ww, int wh, int depth_inv, float* g_prob, float* g_dv,
                                        hipStream_t st);
void launch_composite_layers_bwd(const enerf_composite_layers_bwd_t& g, hipStream_t st);
// the composite frame's camera-only preparation (prep_job.h CompositePrep, geometry.hip k_composite_prep): composite_prep_job checks
// the C arguments and lays the job out (ENERF_EINVAL + message, nothing launched), launch_composite_prep runs it
struct CompositePrep;
int composite_prep_job(const enerf_composite_prep_t* a, CompositePrep* job);
void launch_composite_prep(const CompositePrep& job, hipStream_t st);
// boxes that move (enerf_forward_composite_moving): the windowed kernels with their corners read on the device — xy = (x0, y0) of the
// window, win_xy = (x0, y0) per layer — as the preparation launch resolved them (prep_job.h, MovingBoxes)
void launch_feature_volume_window_at(const float* feat_nhwc, const float* proj, const float* dv, int B, int S, int C, int Hs, int Ws, int D,
                                     int h, int w, const int* xy, int ww, int wh, float* vol, hipStream_t st);
void launch_depth_regression_window_at(const float* prob, const float* dv, int B, int D, int h, int w, const int* xy, int ww, int wh,
                                       int depth_inv, float* depth, float* std, hipStream_t st);
void launch_composite_layers_at(const enerf_composite_layers_t& a, hipStream_t st, const int* invalid, const int* win_xy);
// enerf_composite_layers_at / the moving frame's merge: composite_layers_run with the corners on the device (win_xy == nullptr: as above)
int composite_layers_run_at(const enerf_composite_layers_t* a, const int* invalid, const int* win_xy, hipStream_t st);
// the layers' boxes of a target camera on the device (io.hip k_layer_boxes)
void launch_layer_boxes(const float* bounds, const float* tar_ext, const float* tar_ixt, int L, int H, int W, const int* sizes,
                        float near_min, float* xy, float* near_far, int* flags, hipStream_t st);

}  // namespace enerf
