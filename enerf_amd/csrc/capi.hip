// capi.hip — the extern "C" boundary (include/enerf_hip.h): argument validation, the cost-regularisation
// network driver, error reporting.  No torch types; raw device pointers + sizes + a hipStream_t.
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "kernels.h"
#include "prep_job.h"

using namespace enerf;

namespace enerf {
__global__ __launch_bounds__(256) void k_zero(unsigned* __restrict__ p, long long n) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) p[i] = 0u;
}
void zero_async(void* p, size_t bytes, hipStream_t st) {
    const long long n = (long long)(bytes / 4);
    if (n <= 0) return;
    long long blocks = cdivl(n, 256 * 4);
    if (blocks > 4096) blocks = 4096;
    ENERF_LAUNCH_SIMPLE(k_zero, (unsigned)blocks, 256, 0, st, (unsigned*)p, n);
}
// two accumulators in one launch when the caller allocated them back to back (the Python binding does)
void zero_async2(void* p, size_t bytes_p, void* q, size_t bytes_q, hipStream_t st) {
    if ((char*)p + bytes_p == (char*)q && bytes_p % 4 == 0) { zero_async(p, bytes_p + bytes_q, st); return; }
    zero_async(p, bytes_p, st);
    zero_async(q, bytes_q, st);
}
#ifdef ENERF_EMU
// emulator build only (tests): the CU count the launch geometry is sized by, settable so that the persistent kernels' later passes
// run on CPU too (tests/emu_lib.py emu_cu_count); not part of the C ABI, absent from the product library
static int g_emu_cu_count = 256;
}  // namespace enerf
extern "C" void emu_set_cu_count(int n) { enerf::g_emu_cu_count = n > 0 ? n : 256; }
// the calling thread's launch trace (tests/emu/hip_emu.h; tests/emu_lib.py emu_trace): clear it and switch it on or off; copy it
// out (returns its length: a caller with a smaller buffer asks again)
#ifdef ENERF_EMU_TRACE
extern "C" void emu_trace_reset(int on) { emu::trace().on = on != 0; emu::trace().text.clear(); }
extern "C" long long emu_trace_read(char* buf, long long cap) {
    const std::string& t = emu::trace().text;
    if (buf != nullptr && cap > 0) memcpy(buf, t.data(), t.size() < (size_t)cap ? t.size() : (size_t)cap);
    return (long long)t.size();
}
#endif
namespace enerf {
#endif
int device_cu_count() {
#ifdef ENERF_EMU
    return g_emu_cu_count;
#else
    static int cached[64];                         // per device ordinal; 0 = not queried yet (benign race: same value)
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
    if (cached[dev] == 0) {
        int n = 0;
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
        cached[dev] = n;
    }
    return cached[dev];
#endif
}
}  // namespace enerf

namespace enerf {
static thread_local char g_err[512] = "";
const char* last_error() { return g_err; }
int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}
int check_launch(const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(ENERF_ELAUNCH, "%s: %s", what, hipGetErrorString(e));
    return ENERF_OK;
}
}  // namespace enerf
namespace {

// ---- cost-reg layer table ------------------------------------------------------------------------
// buffers a layer reads / writes: the caller's volume and outputs, and the workspace's activations in the order they are carved
enum { kVol = -1, kNoBuf = -2, kFeatProb = -3, kC0 = 0, kC1, kC2, kC3, kC4, kY9, kY11, kC5, kC6, kY7, kNumBufs };
// idx: the reference's conv number (-1: the fused heads, 8 -> 8 + 1, last); div: the input volume is (D, h, w) / div
struct LayerSpec { int idx, cin, cout, kind, relu, in, res, out, div; };
int costreg_layers(int cin0, int full, LayerSpec* L) {
    int n = 0;
    L[n++] = {0, cin0, 8, kConvS1, 1, kVol, kNoBuf, kC0, 1};
    L[n++] = {1, 8, 16, kConvS2, 1, kC0, kNoBuf, kC1, 1};
    L[n++] = {2, 16, 16, kConvS1, 1, kC1, kNoBuf, kC2, 2};
    L[n++] = {3, 16, 32, kConvS2, 1, kC2, kNoBuf, kC3, 2};
    L[n++] = {4, 32, 32, kConvS1, 1, kC3, kNoBuf, kC4, 4};
    if (full) {
        L[n++] = {5, 32, 64, kConvS2, 1, kC4, kNoBuf, kC5, 4};
        L[n++] = {6, 64, 64, kConvS1, 1, kC5, kNoBuf, kC6, 8};
        L[n++] = {7, 64, 32, kConvT2, 0, kC6, kC4, kY7, 8};                     // conv4 + conv7
    }
    L[n++] = {9, 32, 16, kConvT2, 0, full ? kY7 : kC4, kC2, kY9, 4};            // conv2 + conv9
    L[n++] = {11, 16, 8, kConvT2, 0, kY9, kC0, kY11, 2};                        // conv0 + conv11
    L[n++] = {-1, 8, 9, kConvS1, 0, kY11, kNoBuf, kFeatProb, 1};                // feat_conv ++ depth_conv
    return n;
}
// conv0 and the fused heads carry the pk8 and b4 images besides their own
Conv3dImage layer_image(const LayerSpec& s) { return conv3d_layer_image(s.cin, s.cout, s.kind, s.kind == kConvS1 && (s.cout == 8 || s.idx < 0)); }
// floats of every workspace buffer, in carve order; returns how many there are
int costreg_buffers(int full, long long n0, long long* floats) {
    const long long n1 = n0 / 8, n2 = n1 / 8, n3 = n2 / 8;
    const long long f[kNumBufs] = {n0 * 8, n1 * 16, n1 * 16, n2 * 32, n2 * 32, n1 * 16, n0 * 8, n3 * 64, n3 * 64, n2 * 32};
    const int n = full ? kNumBufs : kC5;
    for (int i = 0; i < n; ++i) floats[i] = f[i];
    return n;
}
// What one enerf_cost_reg call runs: every layer's route, decided before anything is launched, and the two layout hand-offs that
// follow from the routes — the cost volume (warp -> conv0) and conv11's output (-> fused heads) travel as channel-quad planes exactly
// when both ends are kernels that speak that layout.
struct CostRegPlan {
    int n;
    LayerSpec spec[12];
    Conv3dRoute route[12];
    bool vol_planar_ok;      // conv0 can read a quad-planar volume
    bool heads_planar;       // conv11 writes, and the heads read, quad planes
};
CostRegPlan cost_reg_plan(int in_channels, int full, int B, int D, int h, int w, const Options& opt, int cus) {
    CostRegPlan P;
    P.n = costreg_layers(in_channels, full, P.spec);
    for (int i = 0; i < P.n; ++i) {
        const LayerSpec& s = P.spec[i];
        P.route[i] = conv3d_route(conv3d_layer_of(layer_image(s), s.cin, s.cout, s.kind), s.res != kNoBuf, s.out == kFeatProb, B,
                                  D / s.div, h / s.div, w / s.div, opt, cus);
    }
    P.vol_planar_ok = conv3d_route_planar_in(P.route[0]);
    P.heads_planar = conv3d_route_planar_out(P.route[P.n - 2]) && conv3d_route_planar_in(P.route[P.n - 1]);
    return P;
}
}  // namespace

extern "C" {

int enerf_abi_version(void) { return ENERF_ABI_VERSION; }
const char* enerf_last_error(void) { return last_error(); }

int enerf_channels_last(const float* src, float* dst, int n, int C, long long P, int Cpad, enerf_stream_t stream) {
    REQUIRE(src && dst && n > 0 && C > 0 && P > 0 && Cpad >= C, "channels_last: bad arguments");
    launch_channels_last(src, dst, n, C, P, Cpad, (hipStream_t)stream);
    return check_launch("channels_last");
}
int enerf_channels_first(const float* src, float* dst, int n, int C, long long P, int Cpad, enerf_stream_t stream) {
    REQUIRE(src && dst && n > 0 && C > 0 && P > 0 && Cpad >= C, "channels_first: bad arguments");
    launch_channels_first(src, dst, n, C, P, Cpad, (hipStream_t)stream);
    return check_launch("channels_first");
}
int enerf_pack_img_feat_rgb(const float* im_feat, int C, int Hf, int Wf, const float* src_inps, int H, int W, int Hr,
                            int Wr, int tex, int n_img, float* out, enerf_stream_t stream) {
    REQUIRE(im_feat && src_inps && out, "pack_img_feat_rgb: null pointer");
    REQUIRE(C > 0 && tex >= C + 3 && tex % 4 == 0 && n_img > 0 && Hr > 0 && Wr > 0, "pack_img_feat_rgb: bad shape");
    launch_pack_img_feat_rgb(im_feat, C, Hf, Wf, src_inps, H, W, Hr, Wr, tex, n_img, out, (hipStream_t)stream);
    return check_launch("pack_img_feat_rgb");
}
int enerf_get_proj_mats(const float* src_ixts, const float* src_exts, const float* tar_ixt, const float* tar_ext, int B,
                        int S, float src_scale, float tar_scale, float* proj, enerf_stream_t stream) {
    REQUIRE(src_ixts && src_exts && tar_ixt && tar_ext && proj && B > 0 && S > 0, "get_proj_mats: bad arguments");
    launch_proj_mats(src_ixts, src_exts, tar_ixt, tar_ext, B, S, src_scale, tar_scale, proj, (hipStream_t)stream);
    return check_launch("get_proj_mats");
}
int enerf_get_depth_values(const float* near_far, const float* prev_depth, const float* prev_std,
                           const float* prev_near_far, int B, int D, int h, int w, int hp, int wp, int depth_inv,
                           float* depth_values, float* near_far_out, enerf_stream_t stream) {
    REQUIRE(depth_values && near_far_out && B > 0 && D > 0 && h > 0 && w > 0, "get_depth_values: bad arguments");
    if (prev_depth) REQUIRE(prev_std && prev_near_far && hp > 0 && wp > 0, "get_depth_values: incomplete previous level");
    else REQUIRE(near_far, "get_depth_values: near_far required at level 0");
    launch_depth_values(near_far, prev_depth, prev_std, prev_near_far, B, D, h, w, hp, wp, depth_inv, depth_values,
                        near_far_out, (hipStream_t)stream);
    return check_launch("get_depth_values");
}
int enerf_level_prep(const float* src_ixts, const float* src_exts, const float* tar_ixt, const float* tar_ext, int B,
                     int S, float src_scale, float tar_scale, float* proj, const float* near_far,
                     const float* prev_depth, const float* prev_std, const float* prev_near_far, int D, int h, int w,
                     int hp, int wp, int depth_inv, float* depth_values, float* near_far_out, enerf_stream_t stream) {
    REQUIRE(src_ixts && src_exts && tar_ixt && tar_ext && proj && B > 0 && S > 0, "level_prep: bad projection arguments");
    REQUIRE(depth_values && near_far_out && D > 0 && h > 0 && w > 0, "level_prep: bad depth arguments");
    if (prev_depth) REQUIRE(prev_std && prev_near_far && hp > 0 && wp > 0, "level_prep: incomplete previous level");
    else REQUIRE(near_far, "level_prep: near_far required at level 0");
    launch_level_prep(src_ixts, src_exts, tar_ixt, tar_ext, S, src_scale, tar_scale, proj, near_far, prev_depth, prev_std,
                      prev_near_far, B, D, h, w, hp, wp, depth_inv, depth_values, near_far_out, (hipStream_t)stream);
    return check_launch("level_prep");
}
int enerf_build_feature_volume(const float* feat, const float* proj, const float* depth_values, int B, int S, int C,
                               int Hs, int Ws, int D, int h, int w, float* vol, enerf_stream_t stream) {
    REQUIRE(feat && proj && depth_values && vol, "build_feature_volume: null pointer");
    REQUIRE(C == 8 || C == 16 || C == 32, "build_feature_volume: C=%d unsupported (8/16/32)", C);
    REQUIRE(B > 0 && S > 0 && Hs > 1 && Ws > 1 && D > 0 && h > 0 && w > 0, "build_feature_volume: bad shape");
    REQUIRE((long long)B * S * Hs * Ws * C < (1LL << 32) && (long long)Hs * Ws < (1LL << 23),
            "build_feature_volume: source features too large for 32-bit gather offsets");
    REQUIRE((long long)B * D * h * w * (C / 4) < (1LL << 31) && (long long)h * w < (1LL << 23),
            "build_feature_volume: volume too large for 32-bit voxel indices");
    // the launch carries (b, d) in gridDim.z and forms the voxel index with 24-bit multiplies (volume.hip, round 4)
    REQUIRE((long long)B * D <= 65535 && (long long)B * D * h < (1LL << 23) && w < (1 << 23),
            "build_feature_volume: B*D=%lld planes / B*D*h=%lld rows beyond the grid-carried voxel decomposition (65535 / 2^23)",
            (long long)B * D, (long long)B * D * h);
    launch_feature_volume(feat, proj, depth_values, B, S, C, Hs, Ws, D, h, w, vol, (hipStream_t)stream);
    return check_launch("build_feature_volume");
}

long long enerf_cost_reg_packed_floats(int in_channels, int full) {
    LayerSpec L[12];
    int n = costreg_layers(in_channels, full, L);
    long long t = 0;
    for (int i = 0; i < n; ++i) t += layer_image(L[i]).floats;
    return t;
}
int enerf_cost_reg_pack(const enerf_costreg_raw_t* raw, float* packed, enerf_stream_t stream) {
    REQUIRE(raw && packed, "cost_reg_pack: null pointer");
    REQUIRE(raw->in_channels == 8 || raw->in_channels == 16 || raw->in_channels == 32, "cost_reg_pack: in_channels");
    hipStream_t st = (hipStream_t)stream;
    LayerSpec L[12];
    int n = costreg_layers(raw->in_channels, raw->full, L);
    float* p = packed;
    for (int i = 0; i < n; ++i) {
        const LayerSpec& s = L[i];
        const Conv3dImage im = layer_image(s);
        const float *w = raw->feat_conv_w, *wd = raw->depth_conv_w;         // the fused heads: no BN (scale / shift = 1 / 0)
        if (s.idx >= 0) {
            const enerf_conv_bn_t& c = raw->conv[s.idx];
            REQUIRE(c.w && c.bn_weight && c.bn_bias && c.bn_mean && c.bn_var, "cost_reg_pack: conv%d missing", s.idx);
            w = c.w; wd = nullptr;
            launch_conv3d_pack(c.w, nullptr, s.cout, c.bn_weight, c.bn_bias, c.bn_mean, c.bn_var, 1e-5f, s.cin, s.cout, s.kind,
                               p + im.w, p + im.scale, p + im.shift, st);
        } else {
            REQUIRE(w && wd, "cost_reg_pack: heads missing");
            launch_conv3d_pack(w, wd, 8, nullptr, nullptr, nullptr, nullptr, 1e-5f, s.cin, s.cout, s.kind, p + im.w, p + im.scale,
                               p + im.shift, st);
        }
        if (im.t2pair >= 0) launch_conv3d_t2_pair_pack(p + im.w, p + im.t2pair, st);      // from the image just packed
        if (im.pk8 >= 0) launch_conv3d_pk8_pack(w, wd, s.cin, p + im.pk8, st);
        if (im.b4 >= 0) launch_conv3d_b4_pack(w, wd, s.cin, p + im.b4, st);
        p += im.floats;
    }
    return check_launch("cost_reg_pack");
}
size_t enerf_cost_reg_workspace_bytes(int full, int B, int D, int h, int w) {
    long long floats[kNumBufs], f = 0;
    const int n = costreg_buffers(full, (long long)B * D * h * w, floats);
    for (int i = 0; i < n; ++i) f += floats[i];
    return (size_t)f * sizeof(float);
}
int enerf_cost_reg(const float* packed, int in_channels, int full, const float* vol, int B, int D, int h, int w,
                   float* feat, float* prob, void* workspace, size_t workspace_bytes, const enerf_options_t* options,
                   enerf_stream_t stream) {
    REQUIRE(feat, "cost_reg: null pointer");
    return cost_reg_run(packed, in_channels, full, vol, 0, B, D, h, w, feat, prob, workspace, workspace_bytes, options,
                        (hipStream_t)stream);
}
int enerf_cost_reg_prob(const float* packed, int in_channels, int full, const float* vol, int B, int D, int h, int w, float* prob,
                        void* workspace, size_t workspace_bytes, const enerf_options_t* options, enerf_stream_t stream) {
    return cost_reg_run(packed, in_channels, full, vol, 0, B, D, h, w, nullptr, prob, workspace, workspace_bytes, options,
                        (hipStream_t)stream);
}
}  // extern "C"
namespace enerf {
bool cost_reg_conv0_planar(const enerf_options_t& o, int in_channels, int full, int B, int D, int h, int w) {
    return cost_reg_plan(in_channels, full, B, D, h, w, o, device_cu_count()).vol_planar_ok;
}
bool cost_reg_feat_optional(const enerf_options_t& o, int in_channels, int full, int B, int D, int h, int w) {
    const CostRegPlan P = cost_reg_plan(in_channels, full, B, D, h, w, o, device_cu_count());
    return conv3d_route_optional_out(P.route[P.n - 1]);
}
int cost_reg_run(const float* packed, int in_channels, int full, const float* vol, int vol_planar, int B, int D, int h, int w,
                 float* feat, float* prob, void* workspace, size_t workspace_bytes, const enerf_options_t* options,
                 hipStream_t st, const CostRegHook* hook) {
    REQUIRE(packed && vol && prob && workspace, "cost_reg: null pointer");
    REQUIRE(in_channels == 8 || in_channels == 16 || in_channels == 32, "cost_reg: in_channels=%d unsupported (8/16/32)",
            in_channels);
    REQUIRE(B > 0 && D > 0 && h > 0 && w > 0, "cost_reg: bad shape");
    int div = full ? 8 : 4;
    REQUIRE(D % div == 0 && h % div == 0 && w % div == 0, "cost_reg: D,h,w (%d,%d,%d) must be divisible by %d", D, h, w, div);
    if (workspace_bytes < enerf_cost_reg_workspace_bytes(full, B, D, h, w))
        return fail(ENERF_EWORKSPACE, "cost_reg: workspace too small");
    const CostRegPlan P = cost_reg_plan(in_channels, full, B, D, h, w, resolve_options(options), device_cu_count());
    if (feat == nullptr && !conv3d_route_optional_out(P.route[P.n - 1]))
        return fail(ENERF_EINVAL, "cost_reg: the heads' kernel at this shape and these options cannot skip the feature output (needs the batched-4x4 heads, conv3d_b4 != 1)");
    if (vol_planar && !P.vol_planar_ok)
        return fail(ENERF_EINVAL, "cost_reg: a quad-planar volume needs the asynchronously staged conv0 kernel (conv3d_b4 0/2, D % 4 == 0, >= conv3d_lds_min_voxels)");
    float* buf[kNumBufs] = {};
    long long floats[kNumBufs];
    const int nbuf = costreg_buffers(full, (long long)B * D * h * w, floats);
    float* ws = (float*)workspace;
    for (int i = 0; i < nbuf; ++i) { buf[i] = ws; ws += floats[i]; }
    bool ok = true;
    const float* p = packed;
    for (int i = 0; i < P.n; ++i) {
        const LayerSpec& s = P.spec[i];
        const Conv3dImage im = layer_image(s);
        Conv3dDesc d = conv3d_desc(p, im, s.cin, s.cout, s.kind, s.relu);
        p += im.floats;
        d.in_planar = i == 0 ? vol_planar : (i == P.n - 1 && P.heads_planar);
        d.out_planar = i == P.n - 2 && P.heads_planar;
        const bool last = s.out == kFeatProb;
        ok &= launch_conv3d(d, P.route[i], s.in == kVol ? vol : buf[s.in], s.res == kNoBuf ? nullptr : buf[s.res], last ? feat : buf[s.out],
                            last ? prob : nullptr, B, D / s.div, h / s.div, w / s.div, st);
        if (hook != nullptr && hook->after_layer == s.idx) hook->fn(hook->ctx);      // (conv0 .. conv2: the table's first three rows)
    }
    if (!ok) return fail(ENERF_EINVAL, "cost_reg: a layer shape has no kernel (in_channels=%d full=%d)", in_channels, full);
    return check_launch("cost_reg");
}
}  // namespace enerf
#ifdef ENERF_EMU
// emulator build only (tests/test_conv3d_routes.py): the plan of a whole cost-reg network as text, one "name<template values>" per
// layer in launch order, then "vol_planar=0|1" and "heads_planar=0|1", newline-separated; launches nothing.  Returns the length
// (a caller with a smaller buffer asks again).
extern "C" long long emu_cost_reg_routes(int in_channels, int full, int B, int D, int h, int w, const enerf_options_t* options,
                                         int cu_count, char* buf, long long cap) {
    const CostRegPlan P = cost_reg_plan(in_channels, full, B, D, h, w, resolve_options(options), cu_count);
    std::string t;
    char name[64];
    for (int i = 0; i < P.n; ++i) {
        conv3d_route_name(P.route[i], name, sizeof(name));
        t += name;
        t += "\n";
    }
    t += P.vol_planar_ok ? "vol_planar=1\n" : "vol_planar=0\n";
    t += P.heads_planar ? "heads_planar=1\n" : "heads_planar=0\n";
    if (buf != nullptr && cap > 0) memcpy(buf, t.data(), t.size() < (size_t)cap ? t.size() : (size_t)cap);
    return (long long)t.size();
}
// emulator build only (tests/test_wgrad_routes.py): the route of one weight gradient as text — "name<template values>", then
// key=value lines for scratch_bytes, atomic, second_stage, blocks, cols, chunks, tiles_a, tiles_b, tiles_y, tiles_x; launches nothing.
// shape: the 20 fields of WgradShape in order.  Returns the length.
extern "C" long long emu_wgrad_route(const int* shape, int a16, int b16, long long workspace_bytes, int cu_count, char* buf, long long cap) {
    const int* s = shape;
    const WgradShape p = {s[0], s[1], s[2], s[3], s[4], s[5], s[6], s[7], s[8], s[9], s[10], s[11], s[12], s[13], s[14], s[15], s[16], s[17], s[18], s[19] != 0};
    const WgradRoute r = wgrad_route(p, a16 != 0, b16 != 0, (size_t)workspace_bytes, cu_count);
    char name[64], text[512];
    wgrad_route_name(r, name, sizeof(name));
    const int n = snprintf(text, sizeof(text), "%s\nscratch_bytes=%zu\natomic=%d\nsecond_stage=%s\nblocks=%d\ncols=%d\nchunks=%d\ntiles_a=%d\ntiles_b=%d\ntiles_y=%d\ntiles_x=%d\n",
                           name, r.scratch_bytes, (int)r.atomic, wgrad_route_second_stage(r), r.blocks, r.cols, r.chunks, r.tiles_a, r.tiles_b, r.tiles_y, r.tiles_x);
    if (buf != nullptr && cap > 0) memcpy(buf, text, n < cap ? n : cap);
    return n;
}
#endif
extern "C" {

int enerf_depth_regression(const float* prob, const float* depth_values, int B, int D, int h, int w, int depth_inv,
                           float* depth, float* std, enerf_stream_t stream) {
    REQUIRE(prob && depth_values && depth && std && B > 0 && D > 0 && h > 0 && w > 0, "depth_regression: bad arguments");
    launch_depth_regression(prob, depth_values, B, D, h, w, depth_inv, depth, std, nullptr, (hipStream_t)stream);
    return check_launch("depth_regression");
}
int enerf_build_rays(const float* rays8, const float* depth, const float* std, const float* near_far, int B, int N,
                     int h, int w, int Hr, int Wr, int depth_inv, float* rays12, enerf_stream_t stream) {
    if (N == 0 && B > 0) return ENERF_OK;
    REQUIRE(rays8 && depth && std && near_far && rays12, "build_rays: null pointer");
    REQUIRE(B > 0 && N >= 0 && h > 0 && w > 0 && Hr >= h && Wr >= w, "build_rays: bad shape");
    launch_build_rays(rays8, depth, std, near_far, B, N, h, w, Hr, Wr, depth_inv, rays12, (hipStream_t)stream);
    return check_launch("build_rays");
}

long long enerf_nerf_packed_floats(int F) { return nerf_packed_floats(F); }
int enerf_nerf_pack(const enerf_nerf_raw_t* raw, int F, int viewdir_agg, float* packed, enerf_stream_t stream) {
    REQUIRE(raw && packed, "nerf_pack: null pointer");
    REQUIRE(F == 11 || F == 35, "nerf_pack: F=%d unsupported (feat_ch+3 must be 11 or 35)", F);
    REQUIRE(raw->glob_w && raw->glob_b && raw->aggw_w && raw->aggw_b && raw->fc_w && raw->fc_b && raw->lr0_w &&
                raw->lr0_b && raw->sigma_w && raw->sigma_b && raw->col0_w && raw->col0_b && raw->col2_w && raw->col2_b,
            "nerf_pack: missing parameter");
    if (viewdir_agg) REQUIRE(raw->view_w && raw->view_b, "nerf_pack: view_fc missing");
    launch_nerf_pack(*raw, F, viewdir_agg, packed, (hipStream_t)stream);
    return check_launch("nerf_pack");
}
int enerf_render_rays(const enerf_render_args_t* a, enerf_stream_t stream) {
    REQUIRE(a, "render_rays: null args");
    if (a->N == 0 && a->B > 0) return ENERF_OK;              // empty ray list (e.g. an all-false mask_at_box)
    REQUIRE((a->rays12 || a->rays8) && a->tex && a->vol && a->src_exts && a->src_ixts && a->tar_ext && a->packed &&
                a->rgb && a->depth && a->weights, "render_rays: null pointer");
    if (a->rays8)
        REQUIRE(a->depth_map && a->std_map && a->nf_map && a->map_h > 0 && a->map_w > 0,
                "render_rays: fused build_rays needs depth/std/near_far maps and their size");
    REQUIRE(a->B > 0 && a->N >= 0 && a->Hr > 1 && a->Wr > 1 && a->D > 0 && a->h > 0 && a->w > 0, "render_rays: bad shape");
    if (a->ray_index) REQUIRE(a->ray_count && a->B == 1, "render_rays: ray_index needs ray_count and B == 1");
    if (a->N == 0) return ENERF_OK;
    int rc = launch_render_rays(*a, (hipStream_t)stream);
    if (rc != 0)
        return fail(ENERF_EINVAL, "render_rays: unsupported configuration (code %d: F=%d S=%d n_samples=%d B=%d)", rc,
                    a->F, a->S, a->n_samples, a->B);
    return check_launch("render_rays");
}


}  // extern "C"
namespace enerf {
// ---- the composite network: window check and the preparation job, then its entries (include/enerf_hip.h) ----
static int check_window(const char* what, int h, int w, int x0, int y0, int ww, int wh) {
    REQUIRE(h > 0 && w > 0 && ww > 0 && wh > 0 && x0 >= 0 && y0 >= 0 && (long long)x0 + ww <= w && (long long)y0 + wh <= h,
            "%s: window (x0 %d, y0 %d, %d x %d) outside the %d x %d grid", what, x0, y0, ww, wh, w, h);
    return ENERF_OK;
}
// enerf_composite_prep's arguments -> the job k_composite_prep runs: one block-range per set of planes and per window
int composite_prep_job(const enerf_composite_prep_t* a, CompositePrep* job) {
    REQUIRE(a && job, "composite_prep: null args");
    REQUIRE(a->L >= 1 && a->L <= ENERF_MAX_FG_LAYERS, "composite_prep: L=%d foreground layers unsupported (1..%d)", a->L, ENERF_MAX_FG_LAYERS);
    REQUIRE(a->S >= 1 && a->num_levels >= 1 && a->num_levels <= ENERF_MAX_LEVELS, "composite_prep: S=%d, num_levels=%d unsupported (S >= 1, 1..%d levels)",
            a->S, a->num_levels, ENERF_MAX_LEVELS);
    REQUIRE(a->src_ixts && a->src_exts && a->tar_ixt && a->tar_ext && a->near_far, "composite_prep: null camera / near_far pointer");
    REQUIRE(a->fg_planes > 0 && a->bg_planes > 0 && a->h > 0 && a->w > 0, "composite_prep: planes (%d, %d) / grid %d x %d empty", a->fg_planes,
            a->bg_planes, a->w, a->h);
    REQUIRE((long long)(a->fg_planes > a->bg_planes ? a->fg_planes : a->bg_planes) * a->h * a->w < (1LL << 31), "composite_prep: grid too large");
    CompositePrep& J = *job;
    memset(&J, 0, sizeof(J));
    for (int i = 0; i < a->num_levels; ++i) {
        REQUIRE(a->proj[i], "composite_prep: proj[%d] is null", i);
        J.pj[i] = ProjJob{a->src_ixts, a->src_exts, a->tar_ixt, a->tar_ext, a->proj[i], a->S, a->src_scale[i], a->tar_scale[i]};
    }
    int nb = 0;
    J.n_cas = a->L + 1; J.h = a->h; J.w = a->w; J.depth_inv = a->depth_inv;
    for (int c = 0; c <= a->L; ++c) {
        REQUIRE(a->dv[c] && a->nf[c], "composite_prep: dv[%d] / nf[%d] is null", c, c);
        const int D = c < a->L ? a->fg_planes : a->bg_planes;
        const int blocks = composite_prep_job_blocks((long long)D * a->h * a->w, 256);
        J.cas[c] = CompositePrep::Planes{a->near_far + 2 * c, a->dv[c], a->nf[c], D, nb, blocks};
        nb += blocks;
    }
    for (int i = 0; i < a->num_levels; ++i) {
        if (a->Hr[i] == 0) continue;
        REQUIRE((long long)a->Hr[i] * a->Wr[i] < (1LL << 31), "composite_prep: ray raster of level %d too large", i);
        for (int l = 0; l < a->L; ++l) {
            const int* wn = a->win[i][l];
            REQUIRE(a->index[i][l] && a->count[i][l], "composite_prep: index[%d][%d] / count[%d][%d] is null", i, l, i, l);
            if (int rc = check_window("composite_prep", a->Hr[i], a->Wr[i], wn[0], wn[1], wn[2], wn[3])) return rc;
            const int blocks = composite_prep_job_blocks((long long)wn[2] * wn[3], 256);
            J.win[J.n_win++] = CompositePrep::Window{wn[0], wn[1], wn[2], wn[3], a->Wr[i], nb, blocks, a->index[i][l], a->count[i][l], i, l};
            nb += blocks;
        }
    }
    J.nblocks = nb;
    return ENERF_OK;
}
}  // namespace enerf
extern "C" {
int enerf_build_feature_volume_window(const float* feat, const float* proj, const float* depth_values, int B, int S, int C, int Hs,
                                      int Ws, int D, int h, int w, int x0, int y0, int ww, int wh, float* vol, enerf_stream_t stream) {
    REQUIRE(feat && proj && depth_values && vol, "build_feature_volume_window: null pointer");
    REQUIRE(C == 16 || C == 32, "build_feature_volume_window: C=%d unsupported (16/32)", C);
    REQUIRE(B > 0 && S > 0 && Hs > 1 && Ws > 1 && D > 0, "build_feature_volume_window: bad shape");
    if (int rc = check_window("build_feature_volume_window", h, w, x0, y0, ww, wh)) return rc;
    REQUIRE(wh % 4 == 0 && ww % 4 == 0 && D % 4 == 0, "build_feature_volume_window: wh, ww, D (%d,%d,%d) must be divisible by 4", wh, ww, D);
    REQUIRE((long long)B * S * Hs * Ws * C < (1LL << 32) && (long long)Hs * Ws < (1LL << 23),
            "build_feature_volume_window: source features too large for 32-bit gather offsets");
    REQUIRE((long long)B * D * h * w * (C / 4) < (1LL << 31) && (long long)h * w < (1LL << 23),
            "build_feature_volume_window: grid too large for 32-bit voxel indices");
    REQUIRE((long long)B * D <= 65535 * 2 && (long long)B * D * h < (1LL << 23) && w < (1 << 23),
            "build_feature_volume_window: B*D=%lld planes / B*D*h=%lld rows beyond the grid-carried voxel decomposition",
            (long long)B * D, (long long)B * D * h);
    launch_feature_volume_window(feat, proj, depth_values, B, S, C, Hs, Ws, D, h, w, x0, y0, ww, wh, vol, (hipStream_t)stream);
    return check_launch("build_feature_volume_window");
}
int enerf_depth_regression_window(const float* prob, const float* depth_values, int B, int D, int h, int w, int x0, int y0, int ww,
                                  int wh, int depth_inv, float* depth, float* std, enerf_stream_t stream) {
    REQUIRE(prob && depth_values && depth && std, "depth_regression_window: null pointer");
    REQUIRE(B > 0 && D > 0 && D <= 64, "depth_regression_window: B=%d, D=%d unsupported (D in 1..64)", B, D);
    if (int rc = check_window("depth_regression_window", h, w, x0, y0, ww, wh)) return rc;
    REQUIRE(wh % 4 == 0 && ww % 4 == 0 && D % 4 == 0, "depth_regression_window: wh, ww, D (%d,%d,%d) must be divisible by 4", wh, ww, D);
    REQUIRE((long long)B * D * h * w < (1LL << 31), "depth_regression_window: grid too large");
    launch_depth_regression_window(prob, depth_values, B, D, h, w, x0, y0, ww, wh, depth_inv, depth, std, (hipStream_t)stream);
    return check_launch("depth_regression_window");
}
int enerf_build_feature_volume_window_bwd(const float* feat, const float* proj, const float* depth_values, const float* grad_vol, int B,
                                          int S, int C, int Hs, int Ws, int D, int h, int w, int x0, int y0, int ww, int wh,
                                          float* grad_feat, float* grad_depth_values, enerf_stream_t stream) {
    REQUIRE(feat && proj && depth_values && grad_vol && grad_feat && grad_depth_values, "build_feature_volume_window_bwd: null pointer");
    REQUIRE(C == 16 || C == 32, "build_feature_volume_window_bwd: C=%d unsupported (16/32)", C);
    REQUIRE(B > 0 && S > 0 && Hs > 1 && Ws > 1 && D > 0, "build_feature_volume_window_bwd: bad shape");
    if (int rc = check_window("build_feature_volume_window_bwd", h, w, x0, y0, ww, wh)) return rc;
    REQUIRE(wh % 4 == 0 && ww % 4 == 0 && D % 4 == 0, "build_feature_volume_window_bwd: wh, ww, D (%d,%d,%d) must be divisible by 4", wh, ww,
            D);
    REQUIRE((long long)B * S * Hs * Ws * C < (1LL << 31), "build_feature_volume_window_bwd: feature maps of %lld floats (limit 2^31)",
            (long long)B * S * Hs * Ws * C);
    REQUIRE((long long)B * D * h * w * (C / 4) < (1LL << 31), "build_feature_volume_window_bwd: grid too large for 32-bit voxel indices");
    zero_async2(grad_feat, (size_t)B * S * Hs * Ws * C * sizeof(float), grad_depth_values, (size_t)B * D * h * w * sizeof(float),
                (hipStream_t)stream);
    launch_feature_volume_window_bwd(feat, proj, depth_values, grad_vol, B, S, C, Hs, Ws, D, h, w, x0, y0, ww, wh, grad_feat,
                                     grad_depth_values, (hipStream_t)stream);
    return check_launch("build_feature_volume_window_bwd");
}
int enerf_depth_regression_window_bwd(const float* prob, const float* depth_values, const float* grad_depth, const float* grad_std,
                                      int B, int D, int h, int w, int x0, int y0, int ww, int wh, int depth_inv, float* grad_prob,
                                      float* grad_depth_values, enerf_stream_t stream) {
    REQUIRE(prob && depth_values && grad_depth && grad_std && grad_prob && grad_depth_values, "depth_regression_window_bwd: null pointer");
    REQUIRE(B > 0 && D > 0 && D <= 64, "depth_regression_window_bwd: B=%d, D=%d unsupported (D in 1..64)", B, D);
    if (int rc = check_window("depth_regression_window_bwd", h, w, x0, y0, ww, wh)) return rc;
    REQUIRE(wh % 4 == 0 && ww % 4 == 0 && D % 4 == 0, "depth_regression_window_bwd: wh, ww, D (%d,%d,%d) must be divisible by 4", wh, ww, D);
    REQUIRE((long long)B * D * h * w < (1LL << 31), "depth_regression_window_bwd: grid too large");
    launch_depth_regression_window_bwd(prob, depth_values, grad_depth, grad_std, B, D, h, w, x0, y0, ww, wh, depth_inv, grad_prob,
                                       grad_depth_values, (hipStream_t)stream);
    return check_launch("depth_regression_window_bwd");
}
int enerf_composite_layers_bwd(const enerf_composite_layers_bwd_t* g, enerf_stream_t stream) {
    REQUIRE(g, "composite_layers_bwd: null args");
    const enerf_composite_layers_t* a = &g->fwd;
    REQUIRE(a->L >= 1 && a->L <= ENERF_MAX_FG_LAYERS && a->Ns >= 1 && a->L * a->Ns <= 16,
            "composite_layers_bwd: L=%d foreground layers x %d samples unsupported (L in 1..%d, L*n_samples <= 16)", a->L, a->Ns,
            ENERF_MAX_FG_LAYERS);
    REQUIRE(a->H > 0 && a->W > 0 && (long long)a->H * a->W * (a->L + 1) * a->Ns * 4 < (1LL << 31), "composite_layers_bwd: bad image size");
    REQUIRE(a->bg_raw && a->bg_z && g->grad_bg_raw, "composite_layers_bwd: null pointer");       // grad_rgb / _depth / _weights: NULL = zeros
    REQUIRE(((uintptr_t)a->bg_raw | (uintptr_t)g->grad_bg_raw) % 16 == 0, "composite_layers_bwd: bg_raw / grad_bg_raw must be 16-byte aligned");
    for (int l = 0; l < a->L; ++l) {
        REQUIRE(a->fg_raw[l] && a->fg_z[l] && g->grad_fg_raw[l], "composite_layers_bwd: layer %d: null pointer", l);
        REQUIRE(((uintptr_t)a->fg_raw[l] | (uintptr_t)g->grad_fg_raw[l]) % 16 == 0,
                "composite_layers_bwd: layer %d: fg_raw / grad_fg_raw must be 16-byte aligned", l);
        if (int rc = check_window("composite_layers_bwd", a->H, a->W, a->win[l][0], a->win[l][1], a->win[l][2], a->win[l][3])) return rc;
    }
    launch_composite_layers_bwd(*g, (hipStream_t)stream);
    return check_launch("composite_layers_bwd");
}
int enerf_window_ray_index(int x0, int y0, int ww, int wh, int Hr, int Wr, int* index, int* count, enerf_stream_t stream) {
    REQUIRE(index && count, "window_ray_index: null pointer");
    if (int rc = check_window("window_ray_index", Hr, Wr, x0, y0, ww, wh)) return rc;
    REQUIRE((long long)Hr * Wr < (1LL << 31), "window_ray_index: ray raster too large");
    launch_window_ray_index(x0, y0, ww, wh, Wr, index, count, (hipStream_t)stream);
    return check_launch("window_ray_index");
}
int enerf_render_rays_raw(const enerf_render_raw_args_t* a, enerf_stream_t stream) {
    REQUIRE(a, "render_rays_raw: null args");
    if (a->N == 0 && a->B > 0) return ENERF_OK;
    REQUIRE((a->rays12 || a->rays8) && a->tex && a->src_exts && a->src_ixts && a->tar_ext && a->packed && a->raw && a->z,
            "render_rays_raw: null pointer");
    if (a->rays8)
        REQUIRE(a->depth_map && a->std_map && a->nf_map && a->map_h > 0 && a->map_w > 0,
                "render_rays_raw: fused build_rays needs depth/std/near_far maps and their size");
    REQUIRE(a->B > 0 && a->N >= 0 && a->Hr > 1 && a->Wr > 1, "render_rays_raw: bad shape");
    if (a->vol) REQUIRE(a->D > 0 && a->h > 0 && a->w > 0, "render_rays_raw: bad volume shape");
    if (a->ray_index) REQUIRE(a->ray_count && a->B == 1, "render_rays_raw: ray_index needs ray_count and B == 1");
    enerf_render_args_t r = {};
    r.rays12 = a->rays12; r.tex = a->tex; r.vol = a->vol; r.src_exts = a->src_exts; r.src_ixts = a->src_ixts; r.tar_ext = a->tar_ext;
    r.packed = a->packed; r.rgb = a->raw; r.depth = a->z; r.weights = nullptr;
    r.B = a->B; r.N = a->N; r.S = a->S; r.n_samples = a->n_samples; r.depth_inv = a->depth_inv; r.Hr = a->Hr; r.Wr = a->Wr; r.F = a->F;
    r.D = a->vol ? a->D : 1; r.h = a->vol ? a->h : 1; r.w = a->vol ? a->w : 1;      // (the placement arithmetic still runs; nothing is read)
    r.render_scale = a->render_scale;
    r.rays8 = a->rays8; r.depth_map = a->depth_map; r.std_map = a->std_map; r.nf_map = a->nf_map; r.map_h = a->map_h; r.map_w = a->map_w;
    r.ray_index = a->ray_index; r.ray_count = a->ray_count; r.max_blocks = a->max_blocks;
    const int rc = launch_render_rays_raw(r, (hipStream_t)stream);
    if (rc != 0)
        return fail(ENERF_EINVAL, "render_rays_raw: unsupported configuration (code %d: F=%d S=%d n_samples=%d B=%d)", rc, a->F, a->S,
                    a->n_samples, a->B);
    return check_launch("render_rays_raw");
}
int enerf_composite_layers(const enerf_composite_layers_t* a, enerf_stream_t stream) {
    return enerf::composite_layers_run(a, nullptr, (hipStream_t)stream);
}
}  // extern "C"
namespace enerf {
int composite_layers_run(const enerf_composite_layers_t* a, const int* invalid, hipStream_t stream) {
    return composite_layers_run_at(a, invalid, nullptr, stream);
}
// win_xy != nullptr: the corners a.win[l][0..1] are ignored (checked as 0) and read from the device
int composite_layers_run_at(const enerf_composite_layers_t* a, const int* invalid, const int* win_xy, hipStream_t stream) {
    REQUIRE(a, "composite_layers: null args");
    REQUIRE(a->L >= 1 && a->L <= ENERF_MAX_FG_LAYERS && a->Ns >= 1 && a->L * a->Ns <= 16,
            "composite_layers: L=%d foreground layers x %d samples unsupported (L in 1..%d, L*n_samples <= 16)", a->L, a->Ns,
            ENERF_MAX_FG_LAYERS);
    REQUIRE(a->H > 0 && a->W > 0 && (long long)a->H * a->W * (a->L + 1) * a->Ns * 4 < (1LL << 31), "composite_layers: bad image size");
    REQUIRE(a->bg_raw && a->bg_z && a->rgb && a->depth && a->weights && a->net_output && a->z_vals, "composite_layers: null pointer");
    REQUIRE(((uintptr_t)a->bg_raw | (uintptr_t)a->net_output) % 16 == 0, "composite_layers: bg_raw / net_output must be 16-byte aligned");
    for (int l = 0; l < a->L; ++l) {
        REQUIRE(a->fg_raw[l] && a->fg_z[l], "composite_layers: layer %d: null pointer", l);
        REQUIRE((uintptr_t)a->fg_raw[l] % 16 == 0, "composite_layers: layer %d: fg_raw must be 16-byte aligned", l);
        if (int rc = check_window("composite_layers", a->H, a->W, win_xy ? 0 : a->win[l][0], win_xy ? 0 : a->win[l][1], a->win[l][2],
                                  a->win[l][3]))
            return rc;
    }
    if (win_xy != nullptr) launch_composite_layers_at(*a, stream, invalid, win_xy);
    else launch_composite_layers(*a, stream, invalid);
    return check_launch("composite_layers");
}
}  // namespace enerf
extern "C" {
int enerf_composite_prep(const enerf_composite_prep_t* a, enerf_stream_t stream) {
    CompositePrep job;
    if (int rc = composite_prep_job(a, &job)) return rc;
    launch_composite_prep(job, (hipStream_t)stream);
    return check_launch("composite_prep");
}
int enerf_composite_prep_indexed(const enerf_composite_prep_t* a, const int* view_idx, int V, float* cam_exts, float* cam_ixts,
                                 enerf_stream_t stream) {
    CompositePrep job;
    if (int rc = composite_prep_job(a, &job)) return rc;
    REQUIRE(view_idx && cam_exts && cam_ixts, "composite_prep_indexed: view_idx / cam_exts / cam_ixts is null");
    REQUIRE(V >= 1, "composite_prep_indexed: V=%d views in the camera tables", V);
    job.view_idx = view_idx; job.V = V; job.cam_exts = cam_exts; job.cam_ixts = cam_ixts;
    launch_composite_prep(job, (hipStream_t)stream);
    return check_launch("composite_prep_indexed");
}
// ---- the windowed kernels with their corners on the device (boxes that move).  What the host can check of a window is its size;
// the corner is the caller's promise: 0 <= x0 <= w - ww, 0 <= y0 <= h - wh, as the moving frame's preparation launch leaves it ----
int enerf_build_feature_volume_window_at(const float* feat, const float* proj, const float* depth_values, int B, int S, int C, int Hs,
                                         int Ws, int D, int h, int w, const int* xy, int ww, int wh, float* vol, enerf_stream_t stream) {
    REQUIRE(feat && proj && depth_values && vol, "build_feature_volume_window_at: null pointer");
    REQUIRE(xy, "build_feature_volume_window_at: null xy (two int32 on the device: the window's corner)");
    REQUIRE(C == 16 || C == 32, "build_feature_volume_window_at: C=%d unsupported (16/32)", C);
    REQUIRE(B > 0 && S > 0 && Hs > 1 && Ws > 1 && D > 0, "build_feature_volume_window_at: bad shape");
    if (int rc = check_window("build_feature_volume_window_at", h, w, 0, 0, ww, wh)) return rc;
    REQUIRE(wh % 4 == 0 && ww % 4 == 0 && D % 4 == 0, "build_feature_volume_window_at: wh, ww, D (%d,%d,%d) must be divisible by 4", wh, ww, D);
    REQUIRE((long long)B * S * Hs * Ws * C < (1LL << 32) && (long long)Hs * Ws < (1LL << 23),
            "build_feature_volume_window_at: source features too large for 32-bit gather offsets");
    REQUIRE((long long)B * D * h * w * (C / 4) < (1LL << 31) && (long long)h * w < (1LL << 23),
            "build_feature_volume_window_at: grid too large for 32-bit voxel indices");
    REQUIRE((long long)B * D <= 65535 * 2 && (long long)B * D * h < (1LL << 23) && w < (1 << 23),
            "build_feature_volume_window_at: B*D=%lld planes / B*D*h=%lld rows beyond the grid-carried voxel decomposition",
            (long long)B * D, (long long)B * D * h);
    launch_feature_volume_window_at(feat, proj, depth_values, B, S, C, Hs, Ws, D, h, w, xy, ww, wh, vol, (hipStream_t)stream);
    return check_launch("build_feature_volume_window_at");
}
int enerf_depth_regression_window_at(const float* prob, const float* depth_values, int B, int D, int h, int w, const int* xy, int ww,
                                     int wh, int depth_inv, float* depth, float* std, enerf_stream_t stream) {
    REQUIRE(prob && depth_values && depth && std, "depth_regression_window_at: null pointer");
    REQUIRE(xy, "depth_regression_window_at: null xy (two int32 on the device: the window's corner)");
    REQUIRE(B > 0 && D > 0 && D <= 64, "depth_regression_window_at: B=%d, D=%d unsupported (D in 1..64)", B, D);
    if (int rc = check_window("depth_regression_window_at", h, w, 0, 0, ww, wh)) return rc;
    REQUIRE(wh % 4 == 0 && ww % 4 == 0 && D % 4 == 0, "depth_regression_window_at: wh, ww, D (%d,%d,%d) must be divisible by 4", wh, ww, D);
    REQUIRE((long long)B * D * h * w < (1LL << 31), "depth_regression_window_at: grid too large");
    launch_depth_regression_window_at(prob, depth_values, B, D, h, w, xy, ww, wh, depth_inv, depth, std, (hipStream_t)stream);
    return check_launch("depth_regression_window_at");
}
int enerf_composite_layers_at(const enerf_composite_layers_t* a, const int* win_xy, enerf_stream_t stream) {
    REQUIRE(win_xy, "composite_layers_at: null win_xy ((L,2) int32 on the device: the windows' corners)");
    return enerf::composite_layers_run_at(a, nullptr, win_xy, (hipStream_t)stream);
}
int enerf_layer_boxes(const float* bounds, const float* tar_ext, const float* tar_ixt, int L, int H, int W, const int* sizes,
                      float near_min, float* xy, float* near_far, int* flags, enerf_stream_t stream) {
    REQUIRE(bounds && tar_ext && tar_ixt && sizes && xy && near_far && flags, "layer_boxes: null pointer");
    REQUIRE(L >= 1 && L <= ENERF_MAX_FG_LAYERS, "layer_boxes: L=%d foreground layers unsupported (1..%d)", L, ENERF_MAX_FG_LAYERS);
    REQUIRE(H > 0 && W > 0 && H < (1 << 24) && W < (1 << 24), "layer_boxes: bad image size H=%d W=%d", H, W);
    for (int l = 0; l < L; ++l)
        REQUIRE(sizes[2 * l] > 0 && sizes[2 * l + 1] > 0 && sizes[2 * l] < (1 << 24) && sizes[2 * l + 1] < (1 << 24),
                "layer_boxes: sizes[%d] = (%d, %d) must be positive", l, sizes[2 * l], sizes[2 * l + 1]);
    launch_layer_boxes(bounds, tar_ext, tar_ixt, L, H, W, sizes, near_min, xy, near_far, flags, (hipStream_t)stream);
    return check_launch("layer_boxes");
}

}  // extern "C"

// ---- FeatureNet driver ------------------------------------------------------------------------------
namespace {
struct FLayer { int cin, cout, k, stride, relu; };
// order: conv0.0 conv0.1 conv1.0 conv1.1 conv2.0 conv2.1 toplayer lat1 lat0 smooth1 smooth0
const FLayer kFeat[11] = {{3, 8, 3, 1, 1},  {8, 8, 3, 1, 1},   {8, 16, 5, 2, 1},  {16, 16, 3, 1, 1}, {16, 32, 5, 2, 1},
                          {32, 32, 3, 1, 1}, {32, 32, 1, 1, 0}, {16, 32, 1, 1, 0}, {8, 32, 1, 1, 0},  {32, 16, 3, 1, 0},
                          {32, 8, 3, 1, 0}};
long long flayer_floats(const FLayer& f) { return conv2d_packed_floats(f.cin, f.cout, f.k) + 2 * cdiv(f.cout, 16) * 16; }
}  // namespace

extern "C" {
long long enerf_feature_net_packed_floats(void) {
    long long t = 0;
    for (int i = 0; i < 11; ++i) t += flayer_floats(kFeat[i]);
    // tail: raw lat0 weight (32x8) + bias (32) for the fused smooth0 kernel, smooth0's P/Q image (3072), smooth0's broadcast-A image
    // (round 5: 2 passes x 18 registers x 64 lanes), conv0.0's (4 x 64) and conv0.1's (9 x 64)
    return t + 320 + 3072 + 2304 + 256 + 576;
}
int enerf_feature_net_pack(const enerf_featnet_raw_t* raw, float* packed, enerf_stream_t stream) {
    REQUIRE(raw && packed, "feature_net_pack: null pointer");
    const float* pw[5] = {raw->toplayer_w, raw->lat1_w, raw->lat0_w, raw->smooth1_w, raw->smooth0_w};
    const float* pb[5] = {raw->toplayer_b, raw->lat1_b, raw->lat0_b, raw->smooth1_b, raw->smooth0_b};
    float* p = packed;
    for (int i = 0; i < 11; ++i) {
        const FLayer& f = kFeat[i];
        long long wf = conv2d_packed_floats(f.cin, f.cout, f.k);
        int cp = cdiv(f.cout, 16) * 16;
        if (i < 6) {
            const enerf_conv_bn_t& c = raw->conv[i];
            REQUIRE(c.w && c.bn_weight && c.bn_bias && c.bn_mean && c.bn_var, "feature_net_pack: conv %d missing", i);
            launch_conv2d_pack(c.w, nullptr, c.bn_weight, c.bn_bias, c.bn_mean, c.bn_var, 1e-5f, f.cin, f.cout, f.k, p,
                               p + wf, p + wf + cp, (hipStream_t)stream);
        } else {
            REQUIRE(pw[i - 6] && pb[i - 6], "feature_net_pack: FPN conv %d missing", i);
            launch_conv2d_pack(pw[i - 6], pb[i - 6], nullptr, nullptr, nullptr, nullptr, 1e-5f, f.cin, f.cout, f.k, p,
                               p + wf, p + wf + cp, (hipStream_t)stream);
        }
        p += flayer_floats(f);
    }
    hipMemcpyAsync(p, raw->lat0_w, 256 * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream);
    hipMemcpyAsync(p + 256, raw->lat0_b, 32 * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream);
    zero_async(p + 320, 3072 * sizeof(float), (hipStream_t)stream);                      // reserved (rounds 2-5: smooth0's tap-packed P/Q image)
    launch_conv2d_cb_pack(raw->smooth0_w, 32, 0, 16, p + 320 + 3072, (hipStream_t)stream);          // broadcast-A images (conv2d.hip
    launch_conv2d_cb_pack(raw->smooth0_w, 32, 16, 16, p + 320 + 3072 + 1152, (hipStream_t)stream);  //  k_smooth0_cb, k_conv0_fused_cb)
    launch_conv2d_cb_pack(raw->conv[0].w, 3, 0, 3, p + 320 + 3072 + 2304, (hipStream_t)stream);
    launch_conv2d_cb_pack(raw->conv[1].w, 8, 0, 8, p + 320 + 3072 + 2304 + 256, (hipStream_t)stream);
    return check_launch("feature_net_pack");
}
size_t enerf_feature_net_workspace_bytes(int n_img, int H, int W) {
    long long p0 = (long long)n_img * H * W, p1 = p0 / 4, p2 = p1 / 4;
    // c0a(8) c0(8) f0pre(32) @full ; c1a(16) c1(16) f1pre(32) @half ; c2a(32) c2(32) @quarter
    return (size_t)(p0 * (8 + 8 + 32) + p1 * (16 + 16 + 32) + p2 * (32 + 32)) * sizeof(float);
}
int enerf_feature_net(const float* packed, const float* src_inps, int n_img, int H, int W, float* feat_l0,
                      float* feat_l1, float* feat_l2, int l2_stride, void* workspace, size_t workspace_bytes,
                      const enerf_options_t* options, enerf_stream_t stream) {
    return enerf_feature_net_stage(packed, src_inps, n_img, H, W, feat_l0, feat_l1, feat_l2, l2_stride, workspace,
                                   workspace_bytes, ENERF_FEAT_ALL, options, stream);
}
int enerf_feature_net_stage(const float* packed, const float* src_inps, int n_img, int H, int W, float* feat_l0,
                            float* feat_l1, float* feat_l2, int l2_stride, void* workspace, size_t workspace_bytes,
                            int stage, const enerf_options_t* options, enerf_stream_t stream) {
    return enerf::feature_net_stage_job(packed, src_inps, n_img, H, W, feat_l0, feat_l1, feat_l2, l2_stride, workspace, workspace_bytes,
                                        stage, options, (hipStream_t)stream, nullptr, nullptr);
}
}  // extern "C"
namespace enerf {
int feature_net_stage_job(const float* packed, const float* src_inps, int n_img, int H, int W, float* feat_l0, float* feat_l1,
                          float* feat_l2, int l2_stride, void* workspace, size_t workspace_bytes, int stage,
                          const enerf_options_t* options, hipStream_t stream, const PrepJob* job, int* job_done) {
    if (job_done != nullptr) *job_done = 0;
    const Options opt = resolve_options(options);
    REQUIRE(stage >= ENERF_FEAT_ALL && stage <= ENERF_FEAT_LEVEL2, "feature_net: unknown stage %d", stage);
    const bool trunk = stage == ENERF_FEAT_ALL || stage == ENERF_FEAT_TRUNK;
    const bool lvl1 = stage == ENERF_FEAT_ALL || stage == ENERF_FEAT_LEVEL1;
    const bool lvl2 = stage == ENERF_FEAT_ALL || stage == ENERF_FEAT_LEVEL2;
    REQUIRE(packed && src_inps && feat_l0 && feat_l1 && feat_l2 && workspace, "feature_net: null pointer");
    REQUIRE(n_img > 0 && H > 0 && W > 0 && H % 4 == 0 && W % 4 == 0, "feature_net: H,W (%d,%d) must be divisible by 4", H, W);
    REQUIRE(l2_stride == 8 || l2_stride == 12, "feature_net: l2_stride must be 8 (features) or 12 (texels)");
    if (workspace_bytes < enerf_feature_net_workspace_bytes(n_img, H, W))
        return fail(ENERF_EWORKSPACE, "feature_net: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    Conv2dDesc d[11];
    const float* p = packed;
    for (int i = 0; i < 11; ++i) {
        const FLayer& f = kFeat[i];
        long long wf = conv2d_packed_floats(f.cin, f.cout, f.k);
        int cp = cdiv(f.cout, 16) * 16;
        d[i] = {p, p + wf, p + wf + cp, f.cin, f.cout, f.k, f.stride, f.relu, 0, nullptr, nullptr, nullptr};
        p += flayer_floats(f);
    }
    const long long p0 = (long long)n_img * H * W, p1 = p0 / 4, p2 = p1 / 4;
    const int H1 = H / 2, W1 = W / 2, H2 = H / 4, W2 = W / 4;
    float* ws = (float*)workspace;
    auto take = [&](long long nf) { float* r = ws; ws += nf; return r; };
    float *c0a = take(p0 * 8), *c0 = take(p0 * 8), *f0pre = take(p0 * 32);
    float *c1a = take(p1 * 16), *c1 = take(p1 * 16), *f1pre = take(p1 * 32);
    float *c2a = take(p2 * 32), *c2 = take(p2 * 32);
    int rc = 0;
    if (trunk) {
        if (!opt.featnet_unfused) {
            const bool took = launch_conv0_fused(d[0], d[1], p + 320 + 3072 + 2304, p + 320 + 3072 + 2304 + 256, src_inps, c0, n_img, H, W, st, job);   // conv0.1(conv0.0(image))
            if (took && job_done != nullptr) *job_done = 1;
        } else {
            rc |= launch_conv2d(d[0], src_inps, c0a, nullptr, n_img, H, W, 0, 0, st);  // conv0.0 (NCHW image in)
            rc |= launch_conv2d(d[1], c0a, c0, nullptr, n_img, H, W, 0, 0, st);        // conv0.1
        }
        rc |= launch_conv2d(d[2], c0, c1a, nullptr, n_img, H, W, 0, 0, st);            // conv1.0 (s2)
        rc |= launch_conv2d(d[3], c1a, c1, nullptr, n_img, H1, W1, 0, 0, st);          // conv1.1
        rc |= launch_conv2d(d[4], c1, c2a, nullptr, n_img, H1, W1, 0, 0, st);          // conv2.0 (s2)
        if (!opt.featnet_unfused) {
            d[5].chain_w = d[6].w;                                                     // toplayer (1x1, bias) runs in
            d[5].chain_shift = d[6].shift;                                             // conv2.1's epilogue -> level_0
            rc |= launch_conv2d(d[5], c2a, feat_l0, nullptr, n_img, H2, W2, 0, 0, st);
        } else {
            rc |= launch_conv2d(d[5], c2a, c2, nullptr, n_img, H2, W2, 0, 0, st);      // conv2.1
            rc |= launch_conv2d(d[6], c2, feat_l0, nullptr, n_img, H2, W2, 0, 0, st);  // toplayer  -> level_0
        }
    }
    if (lvl1) {
        if (opt.featnet_unfused || !launch_smooth1_fused(d[7], d[9], c1, feat_l0, f1pre, feat_l1, n_img, H1, W1, st)) {
            rc |= launch_conv2d(d[7], c1, f1pre, feat_l0, n_img, H1, W1, H2, W2, st);      // up2(feat2) + lat1(conv1)
            rc |= launch_conv2d(d[9], f1pre, feat_l1, nullptr, n_img, H1, W1, 0, 0, st);   // smooth1   -> level_1
        }
    }
    if (lvl2) {
        d[10].out_stride = l2_stride;
        d[10].rgb_src = (l2_stride == 12) ? src_inps : nullptr;
        if (!opt.featnet_unfused && !opt.featnet_smooth0_plain) {
            // smooth0(up2(feat1) + lat0(conv0)) in one kernel: the 32-channel full-res sum never touches HBM
            launch_smooth0_fused(d[10], c0, f1pre, p, p + 256, p + 320 + 3072, feat_l2, n_img, H, W, st);
        } else {                                                                       // the two plain 16x16x4-MFMA launches
            rc |= launch_conv2d(d[8], c0, f0pre, f1pre, n_img, H, W, H1, W1, st);      // up2(feat1) + lat0(conv0)
            rc |= launch_conv2d(d[10], f0pre, feat_l2, nullptr, n_img, H, W, 0, 0, st);  // smooth0 -> level_2 / texels
        }
    }
    if (rc != 0) return fail(ENERF_EINVAL, "feature_net: unsupported layer shape");
    return check_launch("feature_net");
}
}  // namespace enerf
extern "C" {
int enerf_pack_texels_cl(const float* feat_cl, int C, const float* src_inps, int H, int W, int Hr, int Wr, int tex,
                         int n_img, float* out, enerf_stream_t stream) {
    REQUIRE(feat_cl && src_inps && out, "pack_texels_cl: null pointer");
    REQUIRE(C > 0 && C % 4 == 0 && tex >= C + 3 && tex % 4 == 0 && n_img > 0 && Hr > 0 && Wr > 0, "pack_texels_cl: bad shape");
    launch_pack_texels_cl(feat_cl, C, src_inps, H, W, Hr, Wr, tex, n_img, out, (hipStream_t)stream);
    return check_launch("pack_texels_cl");
}
}  // extern "C"

extern "C" {
int enerf_gen_rays(const float* tar_ext, const float* tar_ixt, int B, int Hr, int Wr, float scale, float* rays,
                   enerf_stream_t stream) {
    REQUIRE(tar_ext && tar_ixt && rays && B > 0 && Hr > 0 && Wr > 0 && scale > 0.f, "gen_rays: bad arguments");
    launch_gen_rays(tar_ext, tar_ixt, B, Hr, Wr, scale, rays, (hipStream_t)stream);
    return check_launch("gen_rays");
}
int enerf_pack_rgb8(const float* rgb, int H, int W, int flip, unsigned char* out, enerf_stream_t stream) {
    REQUIRE(rgb && out && H > 0 && W > 0, "pack_rgb8: bad arguments");
    launch_pack_rgb8(rgb, H, W, flip, out, (hipStream_t)stream);
    return check_launch("pack_rgb8");
}
int enerf_eval_stats(const float* pred_rgb, const float* gt_rgb, const void* mask, int mask_elem_bytes, long long n_rgb,
                     int img_w, int img_h, int crop_h, int crop_w, const float* pred_depth, const float* gt_depth,
                     long long n_depth, double* acc, enerf_stream_t stream) {
    REQUIRE(acc && n_rgb >= 0 && n_depth >= 0, "eval_stats: bad arguments");
    if (n_rgb > 0) REQUIRE(pred_rgb && gt_rgb, "eval_stats: rgb pointers missing");
    if (n_depth > 0) REQUIRE(pred_depth && gt_depth, "eval_stats: depth pointers missing");
    if (mask) REQUIRE(mask_elem_bytes == 1 || mask_elem_bytes == 4, "eval_stats: mask must be uint8/bool or int32");
    if (img_w > 0) REQUIRE(img_h > 0 && crop_h >= 0 && crop_w >= 0 && n_rgb % ((long long)img_w * img_h) == 0,
                           "eval_stats: crop needs the image extent (n_rgb a multiple of img_w*img_h)");
    zero_async(acc, 6 * sizeof(double), (hipStream_t)stream);
    if (n_rgb + n_depth == 0) return ENERF_OK;
    launch_eval_stats(pred_rgb, gt_rgb, mask, mask_elem_bytes, n_rgb, img_w, img_h, crop_h, crop_w, pred_depth, gt_depth,
                      n_depth, acc, (hipStream_t)stream);
    return check_launch("eval_stats");
}
static int eval_ssim_check_shape(int mask_elem_bytes, int mask_mode, int has_mask, int B, int img_h, int img_w, int rect_mode,
                                 int crop_h, int crop_w) {
    REQUIRE(B > 0 && img_h > 0 && img_w > 0, "eval_ssim: bad arguments (B, img_h, img_w must be positive)");
    REQUIRE(mask_mode == ENERF_SSIM_MASK_GE1 || mask_mode == ENERF_SSIM_MASK_EQ1, "eval_ssim: mask_mode must be 0 (>= 1) or 1 (== 1)");
    REQUIRE(rect_mode == ENERF_SSIM_RECT_NONE || rect_mode == ENERF_SSIM_RECT_CROP || rect_mode == ENERF_SSIM_RECT_BBOX,
            "eval_ssim: rect_mode must be 0 (whole image), 1 (centre crop) or 2 (mask bounding box)");
    if (has_mask) REQUIRE(mask_elem_bytes == 1 || mask_elem_bytes == 4, "eval_ssim: mask must be uint8/bool or int32");
    REQUIRE(has_mask || rect_mode != ENERF_SSIM_RECT_BBOX, "eval_ssim: the bounding-box rectangle needs a mask");
    REQUIRE(img_h >= 7 && img_w >= 7, "eval_ssim: unsupported image extent %dx%d: the 7x7 window exceeds it", img_h, img_w);
    if (rect_mode == ENERF_SSIM_RECT_CROP) {
        REQUIRE(crop_h >= 0 && crop_w >= 0, "eval_ssim: negative crop");
        REQUIRE(img_h - 2LL * crop_h >= 7 && img_w - 2LL * crop_w >= 7,
                "eval_ssim: unsupported crop (%d,%d) of a %dx%d image: the 7x7 window exceeds what is left", crop_h, crop_w,
                img_h, img_w);
    }
    return ENERF_OK;
}
size_t enerf_eval_ssim_workspace_bytes(int B, int img_h, int img_w, int rect_mode, int crop_h, int crop_w) {
    if (eval_ssim_check_shape(1, 0, 1, B, img_h, img_w, rect_mode, crop_h, crop_w) != ENERF_OK) return 0;
    return eval_ssim_workspace_bytes(B, img_h, img_w, rect_mode, crop_h, crop_w);
}
int enerf_eval_ssim(const float* pred_rgb, const float* gt_rgb, const void* mask, int mask_elem_bytes, int mask_mode, int B,
                    int img_h, int img_w, int rect_mode, int crop_h, int crop_w, void* workspace, double* out,
                    enerf_stream_t stream) {
    REQUIRE(pred_rgb && gt_rgb && workspace && out, "eval_ssim: null pointer");
    REQUIRE(((size_t)workspace & 7) == 0 && ((size_t)out & 7) == 0, "eval_ssim: workspace and out must be 8-byte aligned");
    const int rc = eval_ssim_check_shape(mask_elem_bytes, mask_mode, mask != nullptr, B, img_h, img_w, rect_mode, crop_h, crop_w);
    if (rc != ENERF_OK) return rc;
    launch_eval_ssim(pred_rgb, gt_rgb, mask, mask_elem_bytes, mask_mode, B, img_h, img_w, rect_mode, crop_h, crop_w, workspace,
                     out, (hipStream_t)stream);
    return check_launch("eval_ssim");
}
// ---- evaluator LPIPS (csrc/lpips_vgg.h) ----
// the rectangle of the three host-known modes -> {y0, x0, rh, rw}; everything that can be refused without touching the device
static int eval_lpips_rect(const char* who, int mask_elem_bytes, int mask_mode, int has_mask, int B, int img_h, int img_w,
                           int rect_mode, int a, int b, int c, int d, int* rect) {
    REQUIRE(B > 0 && img_h > 0 && img_w > 0, "%s: bad arguments (B, img_h, img_w must be positive)", who);
    REQUIRE(mask_mode == ENERF_SSIM_MASK_GE1 || mask_mode == ENERF_SSIM_MASK_EQ1, "%s: mask_mode must be 0 (>= 1) or 1 (== 1)", who);
    if (has_mask) REQUIRE(mask_elem_bytes == 1 || mask_elem_bytes == 4, "%s: mask must be uint8/bool or int32", who);
    int y0 = 0, x0 = 0, rh = img_h, rw = img_w;
    if (rect_mode == ENERF_SSIM_RECT_CROP) {
        REQUIRE(a >= 0 && b >= 0, "%s: negative crop", who);
        y0 = a; x0 = b; rh = (int)(img_h - 2LL * a); rw = (int)(img_w - 2LL * b);
    } else if (rect_mode == ENERF_LPIPS_RECT_XYWH) {
        x0 = a; y0 = b; rw = c; rh = d;
        REQUIRE(x0 >= 0 && y0 >= 0 && rw > 0 && rh > 0 && (long long)x0 + rw <= img_w && (long long)y0 + rh <= img_h,
                "%s: rectangle x %d y %d w %d h %d lies outside the %dx%d image", who, x0, y0, rw, rh, img_h, img_w);
    } else {
        REQUIRE(rect_mode == ENERF_SSIM_RECT_NONE, "%s: rect_mode must be 0 (whole image), 1 (centre crop) or 3 (x, y, w, h)", who);
    }
    REQUIRE(rh >= 16 && rw >= 16, "%s: unsupported rectangle %dx%d: under 16 pixels the fourth pool leaves nothing for relu5_3", who, rh, rw);
    REQUIRE((long long)2 * B * rh * rw * 64 < (1LL << 31) * 4 && 2 * B <= 65535, "%s: batch too large", who);
    rect[0] = y0; rect[1] = x0; rect[2] = rh; rect[3] = rw;
    return ENERF_OK;
}
long long enerf_lpips_packed_floats(void) { return lpips_packed_floats(); }
int enerf_lpips_pack(const enerf_lpips_raw_t* raw, float* packed, enerf_stream_t stream) {
    REQUIRE(raw && packed, "lpips_pack: null pointer");
    for (int i = 0; i < kVggLayers; ++i) REQUIRE(raw->conv[i].w && raw->conv[i].b, "lpips_pack: conv %d has a null pointer", i);
    for (int l = 0; l < 5; ++l) REQUIRE(raw->lin[l], "lpips_pack: lin%d is null", l);
    launch_lpips_pack(*raw, packed, (hipStream_t)stream);
    return check_launch("lpips_pack");
}
size_t enerf_eval_lpips_workspace_bytes(int B, int img_h, int img_w, int rect_mode, int a, int b, int c, int d) {
    int r[4];
    if (eval_lpips_rect("eval_lpips", 1, 0, 1, B, img_h, img_w, rect_mode, a, b, c, d, r) != ENERF_OK) return 0;
    return eval_lpips_workspace_bytes(B, r[2], r[3]);
}
int enerf_eval_lpips(const float* packed, const float* pred_rgb, const float* gt_rgb, const void* mask, int mask_elem_bytes,
                     int mask_mode, int B, int img_h, int img_w, int rect_mode, int a, int b, int c, int d, void* workspace,
                     size_t workspace_bytes, double* out, enerf_stream_t stream) {
    REQUIRE(packed && pred_rgb && gt_rgb && workspace && out, "eval_lpips: null pointer");
    REQUIRE(((size_t)workspace & 15) == 0 && ((size_t)out & 7) == 0 && ((size_t)packed & 15) == 0,
            "eval_lpips: packed and workspace must be 16-byte aligned, out 8-byte aligned");
    int r[4];
    const int rc = eval_lpips_rect("eval_lpips", mask_elem_bytes, mask_mode, mask != nullptr, B, img_h, img_w, rect_mode, a, b, c, d, r);
    if (rc != ENERF_OK) return rc;
    const size_t need = eval_lpips_workspace_bytes(B, r[2], r[3]);
    if (workspace_bytes < need) return fail(ENERF_EWORKSPACE, "eval_lpips: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    const VggFront f = {pred_rgb, gt_rgb, (const unsigned char*)mask, mask_elem_bytes, mask_mode, B, img_h, img_w, r[0], r[1]};
    launch_eval_lpips(packed, f, r[2], r[3], workspace, out, (hipStream_t)stream);
    return check_launch("eval_lpips");
}
int enerf_lpips_front(const float* packed, const float* pred_rgb, const float* gt_rgb, const void* mask, int mask_elem_bytes,
                      int mask_mode, int B, int img_h, int img_w, int rect_mode, int a, int b, int c, int d, float* out_cl,
                      enerf_stream_t stream) {
    REQUIRE(packed && pred_rgb && gt_rgb && out_cl, "lpips_front: null pointer");
    REQUIRE(((size_t)out_cl & 15) == 0 && ((size_t)packed & 15) == 0, "lpips_front: packed and out_cl must be 16-byte aligned");
    int r[4];
    const int rc = eval_lpips_rect("lpips_front", mask_elem_bytes, mask_mode, mask != nullptr, B, img_h, img_w, rect_mode, a, b, c, d, r);
    if (rc != ENERF_OK) return rc;
    const VggFront f = {pred_rgb, gt_rgb, (const unsigned char*)mask, mask_elem_bytes, mask_mode, B, img_h, img_w, r[0], r[1]};
    launch_vgg_conv3x3(packed, 3, 64, nullptr, out_cl, 2 * B, r[2], r[3], 0, r[2], r[3], 1, &f, (hipStream_t)stream);
    return check_launch("lpips_front");
}
long long enerf_vgg_conv3x3_packed_floats(int cin, int cout) {
    return vgg_conv3x3_supported(cin, cout) ? vgg_conv3x3_packed_floats(cin, cout) : 0;
}
int enerf_vgg_conv3x3_pack(const float* w, const float* b, int cin, int cout, float* packed, enerf_stream_t stream) {
    REQUIRE(w && b && packed, "vgg_conv3x3_pack: null pointer");
    REQUIRE(vgg_conv3x3_supported(cin, cout), "vgg_conv3x3_pack: unsupported layer %d -> %d (not a VGG16 pair)", cin, cout);
    launch_vgg_conv3x3_pack(w, b, cin, cout, packed, (hipStream_t)stream);
    return check_launch("vgg_conv3x3_pack");
}
int enerf_vgg_conv3x3(const float* packed_layer, int cin, int cout, const float* in_cl, float* out_cl, int N, int H, int W,
                      int relu, enerf_stream_t stream) {
    REQUIRE(packed_layer && in_cl && out_cl, "vgg_conv3x3: null pointer");
    REQUIRE(vgg_conv3x3_supported(cin, cout), "vgg_conv3x3: unsupported layer %d -> %d (not a VGG16 pair)", cin, cout);
    REQUIRE(N > 0 && N <= 65535 && H > 0 && W > 0 && (long long)N * H * W * (cin > cout ? cin : cout) < (1LL << 31) * 4,
            "vgg_conv3x3: bad shape (N %d, H %d, W %d)", N, H, W);
    REQUIRE(((size_t)packed_layer & 15) == 0 && ((size_t)out_cl & 15) == 0 && (cin == 3 || ((size_t)in_cl & 15) == 0),
            "vgg_conv3x3: packed_layer, in_cl and out_cl must be 16-byte aligned");
    launch_vgg_conv3x3(packed_layer, cin, cout, in_cl, out_cl, N, H, W, 0, H, W, relu, nullptr, (hipStream_t)stream);
    return check_launch("vgg_conv3x3");
}
int enerf_mask_bbox(const void* mask, int elem_bytes, int mask_mode, int B, int h, int w, int* rect, enerf_stream_t stream) {
    REQUIRE(mask && rect, "mask_bbox: null pointer");
    REQUIRE(elem_bytes == 1 || elem_bytes == 4, "mask_bbox: mask must be uint8/bool or int32");
    REQUIRE(mask_mode == ENERF_SSIM_MASK_GE1 || mask_mode == ENERF_SSIM_MASK_EQ1, "mask_bbox: mask_mode must be 0 (>= 1) or 1 (== 1)");
    REQUIRE(B > 0 && B <= 65535 && h > 0 && w > 0, "mask_bbox: bad shape");
    launch_mask_bbox(mask, elem_bytes, mask_mode, B, h, w, rect, (hipStream_t)stream);
    return check_launch("mask_bbox");
}
// ---- trainer's perceptual term (csrc/perceptual_vgg.h) ----
static int perceptual_check_shape(const char* who, int N, int h, int w) {
    REQUIRE(N > 0 && 2 * (long long)N <= 65535, "%s: N must be 1 .. 32767 image pairs, got %d", who, N);
    REQUIRE(h >= 8 && w >= 8, "%s: unsupported image %dx%d: under 8 pixels the third pool leaves nothing for relu4_3", who, h, w);
    REQUIRE((long long)2 * N * h * w * 64 < (1LL << 31) * 4, "%s: batch too large (N %d of %dx%d)", who, N, h, w);
    return ENERF_OK;
}
long long enerf_perceptual_packed_floats(void) { return perceptual_packed_floats(); }
int enerf_perceptual_pack(const enerf_perceptual_raw_t* raw, float* packed, enerf_stream_t stream) {
    REQUIRE(raw && packed, "perceptual_pack: null pointer");
    for (int i = 0; i < 10; ++i) REQUIRE(raw->conv[i].w && raw->conv[i].b, "perceptual_pack: conv %d has a null pointer", i);
    launch_perceptual_pack(*raw, packed, (hipStream_t)stream);
    return check_launch("perceptual_pack");
}
size_t enerf_perceptual_workspace_bytes(int N, int h, int w) {
    if (perceptual_check_shape("perceptual_workspace_bytes", N, h, w) != ENERF_OK) return 0;
    return perceptual_workspace_bytes(N, h, w);
}
int enerf_perceptual_layout(int N, int h, int w, long long* offsets) {
    REQUIRE(offsets, "perceptual_layout: null pointer");
    const int rc = perceptual_check_shape("perceptual_layout", N, h, w);
    if (rc != ENERF_OK) return rc;
    perceptual_layout(N, h, w, offsets);
    return ENERF_OK;
}
int enerf_perceptual_fwd(const float* packed, const float* pred_rgb, const float* gt_rgb, int N, int h, int w, void* workspace,
                         size_t workspace_bytes, double* out, enerf_stream_t stream) {
    REQUIRE(packed && pred_rgb && gt_rgb && workspace && out, "perceptual_fwd: null pointer");
    REQUIRE(((size_t)workspace & 15) == 0 && ((size_t)out & 7) == 0 && ((size_t)packed & 15) == 0,
            "perceptual_fwd: packed and workspace must be 16-byte aligned, out 8-byte aligned");
    const int rc = perceptual_check_shape("perceptual_fwd", N, h, w);
    if (rc != ENERF_OK) return rc;
    const size_t need = perceptual_workspace_bytes(N, h, w);
    if (workspace_bytes < need) return fail(ENERF_EWORKSPACE, "perceptual_fwd: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    launch_perceptual_fwd(packed, pred_rgb, gt_rgb, N, h, w, workspace, out, (hipStream_t)stream);
    return check_launch("perceptual_fwd");
}
int enerf_perceptual_bwd(const float* packed, int N, int h, int w, void* workspace, size_t workspace_bytes, const float* grad_scale,
                         float* grad_pred, enerf_stream_t stream) {
    REQUIRE(packed && workspace && grad_pred, "perceptual_bwd: null pointer");
    REQUIRE(((size_t)workspace & 15) == 0 && ((size_t)packed & 15) == 0, "perceptual_bwd: packed and workspace must be 16-byte aligned");
    const int rc = perceptual_check_shape("perceptual_bwd", N, h, w);
    if (rc != ENERF_OK) return rc;
    const size_t need = perceptual_workspace_bytes(N, h, w);
    if (workspace_bytes < need) return fail(ENERF_EWORKSPACE, "perceptual_bwd: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    launch_perceptual_bwd(packed, N, h, w, workspace, grad_scale, grad_pred, (hipStream_t)stream);
    return check_launch("perceptual_bwd");
}
long long enerf_vgg_conv3x3_dgrad_packed_floats(int cin, int cout) {
    return vgg_dgrad_supported(cin, cout) ? vgg_dgrad_packed_floats(cin, cout) : 0;
}
int enerf_vgg_conv3x3_dgrad_pack(const float* w, int cin, int cout, float* packed, enerf_stream_t stream) {
    REQUIRE(w && packed, "vgg_conv3x3_dgrad_pack: null pointer");
    REQUIRE(vgg_dgrad_supported(cin, cout), "vgg_conv3x3_dgrad_pack: unsupported layer %d -> %d (not one of the ten trunk layers)", cin, cout);
    launch_vgg_dgrad_pack(w, cin, cout, packed, (hipStream_t)stream);
    return check_launch("vgg_conv3x3_dgrad_pack");
}
int enerf_vgg_conv3x3_dgrad(const float* packed, int cin, int cout, const float* gout_cl, float* gin_cl, int N, int H, int W,
                            enerf_stream_t stream) {
    REQUIRE(packed && gout_cl && gin_cl, "vgg_conv3x3_dgrad: null pointer");
    REQUIRE(vgg_dgrad_supported(cin, cout), "vgg_conv3x3_dgrad: unsupported layer %d -> %d (not one of the ten trunk layers)", cin, cout);
    REQUIRE(N > 0 && N <= 65535 && H > 0 && W > 0 && (long long)N * H * W * (cin > cout ? cin : cout) < (1LL << 31) * 4,
            "vgg_conv3x3_dgrad: bad shape (N %d, H %d, W %d)", N, H, W);
    REQUIRE(((size_t)packed & 15) == 0 && ((size_t)gout_cl & 15) == 0 && (cin == 3 || ((size_t)gin_cl & 15) == 0),
            "vgg_conv3x3_dgrad: packed, gout_cl and gin_cl must be 16-byte aligned");
    launch_vgg_conv3x3_dgrad(packed, cin, cout, gout_cl, gin_cl, N, H, W, (hipStream_t)stream);
    return check_launch("vgg_conv3x3_dgrad");
}
int enerf_gen_rays_at(const float* tar_ext, const float* tar_ixt, const int* xy, int B, int N, float scale, float* rays,
                      enerf_stream_t stream) {
    REQUIRE(tar_ext && tar_ixt && xy && rays && B > 0 && N >= 0 && scale > 0.f, "gen_rays_at: bad arguments");
    if (N == 0) return ENERF_OK;
    launch_gen_rays_at(tar_ext, tar_ixt, xy, B, N, scale, rays, (hipStream_t)stream);
    return check_launch("gen_rays_at");
}
int enerf_rays_bbox_mask(const float* rays, const float* bounds, long long n, int* mask, enerf_stream_t stream) {
    REQUIRE(rays && bounds && mask && n > 0, "rays_bbox_mask: bad arguments");
    launch_rays_bbox_mask(rays, bounds, n, mask, (hipStream_t)stream);
    return check_launch("rays_bbox_mask");
}
int enerf_select_views(const float* cam_points, int V, const float* c2w, int k, int* idx, enerf_stream_t stream) {
    REQUIRE(cam_points && c2w && idx && V > 0 && V <= 1024 && k > 0 && k <= V, "select_views: bad arguments (V <= 1024, k <= V)");
    launch_select_views(cam_points, V, c2w, k, idx, (hipStream_t)stream);
    return check_launch("select_views");
}
int enerf_gather_views(const float* inps, const float* exts, const float* ixts, const int* idx, int k, int H, int W,
                       float* src_inps, float* src_exts, float* src_ixts, enerf_stream_t stream) {
    REQUIRE(inps && exts && ixts && idx && src_inps && src_exts && src_ixts && k > 0 && H > 0 && W > 0 &&
                (long long)k * H * W >= 16LL * k, "gather_views: bad arguments");
    launch_gather_views(inps, exts, ixts, idx, k, H, W, src_inps, src_exts, src_ixts, (hipStream_t)stream);
    return check_launch("gather_views");
}
int enerf_ingest_views_u8(const unsigned char* img, const unsigned char* mask, int dilate, int V, int H, int W, float* out,
                          enerf_stream_t stream) {
    REQUIRE(dilate == 0 || (dilate % 2 == 1 && dilate >= 3 && dilate <= 9), "ingest_views_u8: dilate=%d (0, or an odd box size 3..9)", dilate);
    REQUIRE(V >= 1 && V <= 65535, "ingest_views_u8: V=%d views (1..65535)", V);
    REQUIRE(H >= 1 && W >= 1 && H <= 16 * 65535, "ingest_views_u8: bad image extent %dx%d", H, W);
    REQUIRE(img && out, "ingest_views_u8: null %s", img ? "out" : "img");
    launch_ingest_views_u8(img, mask, dilate, V, H, W, out, (hipStream_t)stream);
    return check_launch("ingest_views_u8");
}
int enerf_ingest_raw_geometry(int Hraw, int Wraw, double input_ratio, int* Hs, int* Ws) {
    REQUIRE(Hs && Ws, "ingest_raw_geometry: null %s", Hs ? "Ws" : "Hs");
    REQUIRE(Hraw >= 1 && Wraw >= 1 && Hraw <= 32768 && Wraw <= 32768, "ingest_raw_geometry: bad raw extent %dx%d (1..32768)", Hraw, Wraw);
    REQUIRE(input_ratio >= 0.25 && input_ratio <= 1.0, "ingest_raw_geometry: input_ratio=%g (0.25..1)", input_ratio);
    ingest_raw_geometry(Hraw, Wraw, input_ratio, Hs, Ws);
    return ENERF_OK;
}
int enerf_ingest_raw_u8(const unsigned char* img, const unsigned char* mask, const float* ixts, const float* dist, int V, int Hraw,
                        int Wraw, double input_ratio, int crop_y, int crop_x, int H, int W, int dilate, unsigned char* mask_scratch,
                        float* out, unsigned char* mask_out, enerf_stream_t stream) {
    REQUIRE(img && out, "ingest_raw_u8: null %s", img ? "out" : "img");
    REQUIRE(V >= 1 && V <= 65535, "ingest_raw_u8: V=%d views (1..65535)", V);
    REQUIRE(Hraw >= 1 && Wraw >= 1 && Hraw <= 32768 && Wraw <= 32768, "ingest_raw_u8: bad raw extent %dx%d (1..32768)", Hraw, Wraw);
    REQUIRE(input_ratio >= 0.25 && input_ratio <= 1.0, "ingest_raw_u8: input_ratio=%g (0.25..1)", input_ratio);   // (NaN fails too)
    REQUIRE(dilate == 0 || (dilate % 2 == 1 && dilate >= 3 && dilate <= 9), "ingest_raw_u8: dilate=%d (0, or an odd box size 3..9)", dilate);
    int Hs = 0, Ws = 0;
    ingest_raw_geometry(Hraw, Wraw, input_ratio, &Hs, &Ws);
    REQUIRE(H >= 1 && W >= 1 && crop_y >= 0 && crop_x >= 0 && crop_y <= Hs - H && crop_x <= Ws - W,
            "ingest_raw_u8: crop (y0=%d, x0=%d, %dx%d) leaves the resized image %dx%d", crop_y, crop_x, H, W, Hs, Ws);
    REQUIRE(dist == nullptr || ixts != nullptr, "ingest_raw_u8: dist without ixts");
    REQUIRE(mask != nullptr || mask_out == nullptr, "ingest_raw_u8: mask_out without a mask");
    REQUIRE(!(dilate > 0 && mask != nullptr && mask_scratch == nullptr), "ingest_raw_u8: dilate=%d with a mask needs mask_scratch (V,Hraw,Wraw)", dilate);
    launch_ingest_raw_u8(img, mask, ixts, dist, V, Hraw, Wraw, input_ratio, crop_y, crop_x, H, W, dilate, mask_scratch, out, mask_out,
                         (hipStream_t)stream);
    return check_launch("ingest_raw_u8");
}
int enerf_bounds_near_far(const float* vertices, int n, const float* tar_ext, int B, float near_min, float* near_far,
                          enerf_stream_t stream) {
    REQUIRE(vertices && tar_ext && near_far, "bounds_near_far: null pointer");
    REQUIRE(B >= 1 && n >= 1, "bounds_near_far: B=%d cameras, n=%d vertices (both >= 1)", B, n);
    launch_bounds_near_far(vertices, n, tar_ext, B, near_min, near_far, (hipStream_t)stream);
    return check_launch("bounds_near_far");
}
}  // extern "C"
