// frame.hip — the whole-frame driver behind enerf_forward / enerf_forward_cached (Network.forward, network.py:76-113 /
// network_human.py:69-119), the device-side mask_at_box compaction (network_human.py:90-93) and the source-view cache.  The cascade
// loop the reference runs in Python is a plan (buffer carving) + ~30 kernel enqueues here, in one C call, with no host
// synchronisation: on the caller's stream, with the leaves of the frame forked onto a side lane (side_lane.h) and joined again.
// Layout: kernels of this file; FeatDims / make_plan (shapes, workspace); FrameRun (one member function per stage) and
// run_frame (their sequence); the composite network's frame in the same form (make_composite_plan, CompositeRun, run_composite:
// enerf_forward_composite); the C entries.
#include <stdint.h>
#include <string.h>

#include "kernels.h"
#include "prep_job.h"
#include "side_lane.h"

using namespace enerf;

namespace enerf {

// =====================================================================================================================
// mask_at_box -> ascending list of selected ray positions (rays[mask_at_box], network_human.py:93).  Three tiny launches:
// per-block counts (1024 elements a block), an exclusive scan of the block counts by one block (also the total),
// and the scatter, which redoes the in-block scan in LDS.  Stable order, so the compacted depth/weights rows match the
// reference's boolean-mask indexing.  HBM-bound byte work: n bytes in, 4*count bytes out.
// =====================================================================================================================
constexpr int kMaskPerThread = 4;
constexpr int kMaskPerBlock = 256 * kMaskPerThread;

__device__ __forceinline__ bool mask_set(const unsigned char* m, int eb, long long i, long long n) {
    if (i >= n) return false;
    if (eb == 1) return m[i] != 0;
    const unsigned char* p = m + i * eb;
    unsigned v = 0;
    for (int k = 0; k < eb; ++k) v |= p[k];
    return v != 0;
}
// in-block exclusive scan of one int per thread (256 threads); returns the block total through `total`
__device__ __forceinline__ int block_exclusive_scan(int v, int* sh, int& total) {
    const int t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {
        const int add = t >= off ? sh[t - off] : 0;
        __syncthreads();
        sh[t] += add;
        __syncthreads();
    }
    total = sh[255];
    const int excl = sh[t] - v;
    __syncthreads();
    return excl;
}
__global__ __launch_bounds__(256) void k_mask_count(const unsigned char* __restrict__ mask, int eb, long long n,
                                                    int* __restrict__ block_counts) {
    __shared__ int sh[256];
    const long long base = (long long)blockIdx.x * kMaskPerBlock + (long long)threadIdx.x * kMaskPerThread;
    int c = 0;
    for (int k = 0; k < kMaskPerThread; ++k) c += mask_set(mask, eb, base + k, n) ? 1 : 0;
    int total;
    block_exclusive_scan(c, sh, total);
    if (threadIdx.x == 0) block_counts[blockIdx.x] = total;
}
__global__ __launch_bounds__(256) void k_mask_scan(const int* __restrict__ block_counts, int nblocks,
                                                   int* __restrict__ block_offsets, int* __restrict__ count) {
    __shared__ int sh[256];
    int carry = 0;
    for (int base = 0; base < nblocks; base += 256) {
        const int i = base + (int)threadIdx.x;
        const int v = i < nblocks ? block_counts[i] : 0;
        int total;
        const int excl = block_exclusive_scan(v, sh, total);
        if (i < nblocks) block_offsets[i] = carry + excl;
        carry += total;
    }
    if (threadIdx.x == 0) count[0] = carry;
}
__global__ __launch_bounds__(256) void k_mask_scatter(const unsigned char* __restrict__ mask, int eb, long long n,
                                                      const int* __restrict__ block_offsets, int* __restrict__ index) {
    __shared__ int sh[256];
    const long long base = (long long)blockIdx.x * kMaskPerBlock + (long long)threadIdx.x * kMaskPerThread;
    bool f[kMaskPerThread];
    int c = 0;
    for (int k = 0; k < kMaskPerThread; ++k) { f[k] = mask_set(mask, eb, base + k, n); c += f[k] ? 1 : 0; }
    int total;
    int o = block_offsets[blockIdx.x] + block_exclusive_scan(c, sh, total);
    for (int k = 0; k < kMaskPerThread; ++k)
        if (f[k]) index[o++] = (int)(base + k);
}
size_t mask_compact_workspace_bytes(long long n) { return (size_t)(2 * cdivl(n > 0 ? n : 1, kMaskPerBlock)) * sizeof(int); }
void launch_mask_compact(const void* mask, int elem_bytes, long long n, int* index, int* count, void* workspace,
                         hipStream_t st) {
    const int nb = (int)cdivl(n, kMaskPerBlock);
    int* counts = (int*)workspace;
    int* offsets = counts + nb;
    const unsigned char* m = (const unsigned char*)mask;
    ENERF_LAUNCH(k_mask_count, (unsigned)nb, 256, 0, st, m, elem_bytes, n, counts);
    ENERF_LAUNCH(k_mask_scan, 1u, 256, 0, st, counts, nb, offsets, count);
    ENERF_LAUNCH(k_mask_scatter, (unsigned)nb, 256, 0, st, m, elem_bytes, n, offsets, index);
}

// =====================================================================================================================
// Source-view gather of a cached frame (enerf_forward_cached; the reference's per-camera gather, zjumocap/enerf_interactive.py:
// 214-217, applied to what the FeatureNet made of the images instead of the images).  For every (b,s) slot of the frame the
// selected view's blocks — one contiguous run per segment: a feature map or a texel image of that view — are copied from the
// cache into the frame's workspace, and the two camera rows with them.  The view index is read here, on the device.
// Pure HBM byte work: grid (x, B*S), a block walks its slot's segments with 16-byte loads and stores, four in flight per thread,
// grid-stride in x.  An index outside [0,V) is never used as an address: the slot is filled with NaN instead.
// =====================================================================================================================
constexpr int kGatherSegs = 6;
struct GatherSeg { const float4* src; float4* dst; long long n4; };    // n4: 16-byte words per view
struct GatherJob {
    GatherSeg seg[kGatherSegs];
    int nseg, V;
    const int* view_idx;                   // (B*S) on the device; nullptr = slot i takes view i (the cache build's camera copy)
    const float *exts, *ixts;              // (V,16), (V,9)
    float *dst_exts, *dst_ixts;            // (B*S,16), (B*S,9), or nullptr = no cameras in this launch
};
__global__ __launch_bounds__(256) void k_gather_sources(GatherJob J) {
    const int img = blockIdx.y;
    const int v = J.view_idx != nullptr ? J.view_idx[img] : img;
    const bool ok = v >= 0 && v < J.V;
    const float qnan = __int_as_float(0x7fc00000);
    const long long stride = (long long)gridDim.x * 256;
    const long long i0 = (long long)blockIdx.x * 256 + threadIdx.x;
    for (int s = 0; s < J.nseg; ++s) {
        const long long n4 = J.seg[s].n4;
        float4* d = J.seg[s].dst + (long long)img * n4;
        if (ok) {
            const float4* p = J.seg[s].src + (long long)v * n4;
            long long i = i0;
            for (; i + 3 * stride < n4; i += 4 * stride) {
                const float4 a = p[i], b = p[i + stride], c = p[i + 2 * stride], e = p[i + 3 * stride];
                d[i] = a; d[i + stride] = b; d[i + 2 * stride] = c; d[i + 3 * stride] = e;
            }
            for (; i < n4; i += stride) d[i] = p[i];
        } else {
            const float4 n = make_float4(qnan, qnan, qnan, qnan);
            for (long long i = i0; i < n4; i += stride) d[i] = n;
        }
    }
    if (blockIdx.x == 0 && J.dst_exts != nullptr && threadIdx.x < 25) {
        const int t = threadIdx.x;
        if (t < 16) J.dst_exts[img * 16 + t] = ok ? J.exts[(long long)v * 16 + t] : qnan;
        else J.dst_ixts[img * 9 + (t - 16)] = ok ? J.ixts[(long long)v * 9 + (t - 16)] : qnan;
    }
}
void launch_gather_sources(const GatherJob& J, int n_img, hipStream_t st) {
    long long most = 1;
    for (int s = 0; s < J.nseg; ++s) most = J.seg[s].n4 > most ? J.seg[s].n4 : most;
    long long gx = cdivl(most, 256 * 4), cap = (long long)device_cu_count() * 8 / n_img;
    if (gx > cap) gx = cap;
    if (gx < 1) gx = 1;
    ENERF_LAUNCH_SIMPLE(k_gather_sources, dim3((unsigned)gx, (unsigned)n_img), 256, 0, st, J);
}

// =====================================================================================================================
// Frame plan: shapes of every level and the carving of the caller's workspace.
// =====================================================================================================================
namespace {
// the FeatureNet's pyramid (feature_net.py:27-36): level_0 at a quarter of the image with 32 channels .. level_2 at full size with 8
struct FeatDims {
    int h[3], w[3], c[3];
    FeatDims(int H, int W) : h{H / 4, H / 2, H}, w{W / 4, W / 2, W}, c{32, 16, 8} {}
    long long pixels(int l) const { return (long long)h[l] * w[l]; }
};
inline int tex_stride(int F) { return 4 * ((F + 3) / 4); }              // floats per render texel: F = C_f + 3, padded to quads
inline int scaled(int n, double s) { return (int)((double)n * s); }      // python: int(H * scale)

// level_2 is only ever the im_feat of a full-resolution render: then the FeatureNet emits it as render texels
int cascade_tex2(const enerf_cascade_t& c) {
    int uses = 0, all_full = 1;
    for (int i = 0; i < c.num; ++i)
        if (c.render_if[i] && c.render_im_feat_level[i] == 2) {
            ++uses;
            all_full &= (c.render_scale[i] == 1.0 && c.im_ibr_scale[i] == 1.0 && c.nerf_model_feat_ch[i] == 8);
        }
    return uses > 0 && all_full && c.num <= 2;
}
inline int l2_stride(int tex2) { return tex2 ? 12 : 8; }                 // floats per pixel of the level-2 map: texels or features
inline int l2_stride(const enerf_cascade_t& c) { return l2_stride(cascade_tex2(c)); }
// level i is rendered straight from the level-2 map (emitted as texels): it has no texel image of its own
inline bool renders_from_l2(const enerf_cascade_t& c, int i, int tex2) {
    return c.render_if[i] && c.render_im_feat_level[i] == 2 && tex2;
}
// render level i reads feature level render_im_feat_level[i]: the channel count must match, and (same_extent: the HIP
// FeatureNet's maps, which are never resampled) so must the extent
int check_render_feat(const char* who, const enerf_cascade_t& c, int i, const FeatDims& fd, int Hr, int Wr, bool same_extent) {
    const int fl = c.render_im_feat_level[i];
    REQUIRE(fl >= 0 && fl <= 2 && fd.c[fl] == c.nerf_model_feat_ch[i],
            "%s: render_im_feat_level[%d]=%d does not have nerf_model_feat_ch=%d channels", who, i, fl, c.nerf_model_feat_ch[i]);
    if (same_extent)
        REQUIRE(fd.h[fl] == Hr && fd.w[fl] == Wr, "%s: level %d renders at %dx%d but feature level_%d is %dx%d "
                "(the HIP FeatureNet path needs render_scale == im_ibr_scale)", who, i, Hr, Wr, fl, fd.h[fl], fd.w[fl]);
    return ENERF_OK;
}

struct LevelPlan {
    int D, h, w, C, Hs, Ws;            // volume extent; cost-volume feature channels and source-map size
    int Hr, Wr, render, masked, F, Ns; // render extent, flags, nerf feature width (C_f + 3), samples per ray
    int fl, from_l2;                   // rendered levels: the feature level of the texels; the texels ARE the level-2 map
    int prob_only;                     // not rendered and the heads' kernel can skip it: no feature volume (no feat3d slot either)
    long long n_rays;
    // workspace offsets (floats)
    size_t proj, dv, nf, vol, feat3d, prob, depth, std, dmvs, tex, rays;
};
struct FramePlan {
    int tex2, hip_feats, cached;
    size_t f[3], featnet_ws, featnet_ws_bytes, costreg_ws, costreg_ws_bytes;
    size_t cam_exts, cam_ixts;                     // cached frame: the gathered (B,S,4,4) / (B,S,3,3) camera rows
    size_t ray_index, ray_count, mask_ws;          // float-sized slots
    LevelPlan L[ENERF_MAX_LEVELS];
    size_t total_floats;
};

// cached: the frame's feature maps, texels and source cameras come from a source cache (enerf_forward_cached): no FeatureNet
// scratch, camera slots instead; every other offset rule is enerf_forward's
int make_plan(const enerf_frame_args_t* a, FramePlan* P, bool cached = false) {
    REQUIRE(a, "forward: null args");
    const enerf_cascade_t& c = a->cas;
    P->cached = cached;
    REQUIRE(c.num >= 1 && c.num <= ENERF_MAX_LEVELS, "forward: cas_config.num=%d unsupported (1..%d)", c.num, ENERF_MAX_LEVELS);
    REQUIRE(a->B > 0 && a->S >= 2 && a->S <= 4 && a->H > 0 && a->W > 0 && a->H % 4 == 0 && a->W % 4 == 0,
            "forward: bad batch shape B=%d S=%d H=%d W=%d (S in 2..4, H and W divisible by 4)", a->B, a->S, a->H, a->W);
    REQUIRE(a->tar_ext && a->tar_ixt && a->near_far, "forward: null batch tensor");
    if (!cached) {
        REQUIRE(a->src_inps && a->src_exts && a->src_ixts, "forward: null batch tensor");
        const int nf = (a->feats_nchw[0] != nullptr) + (a->feats_nchw[1] != nullptr) + (a->feats_nchw[2] != nullptr);
        REQUIRE(nf == 0 || nf == 3, "forward: feats_nchw needs all three levels or none");
        P->hip_feats = nf == 0;
        if (P->hip_feats) REQUIRE(a->feature_net_packed, "forward: feature_net_packed missing");
    } else
        P->hip_feats = 1;                              // the cache holds the HIP FeatureNet's channels-last maps
    P->tex2 = P->hip_feats && cascade_tex2(c);
    size_t off = 0;
    auto take = [&](size_t nfloats) { size_t r = off; off += (nfloats + 63) / 64 * 64; return r; };   // 256-B aligned
    const long long n_img = (long long)a->B * a->S;
    const FeatDims fd(a->H, a->W);
    for (int l = 0; l < 3; ++l) P->f[l] = take((size_t)n_img * fd.pixels(l) * (l == 2 ? l2_stride(P->tex2) : fd.c[l]));
    P->featnet_ws_bytes = P->hip_feats && !cached ? enerf_feature_net_workspace_bytes((int)n_img, a->H, a->W) : 0;
    P->featnet_ws = take(P->featnet_ws_bytes / sizeof(float));
    P->cam_exts = P->cam_ixts = 0;
    if (cached) { P->cam_exts = take((size_t)n_img * 16); P->cam_ixts = take((size_t)n_img * 9); }
    P->costreg_ws_bytes = 0;
    for (int i = 0; i < c.num; ++i) {
        LevelPlan& L = P->L[i];
        memset(&L, 0, sizeof(L));
        L.D = c.volume_planes[i];
        L.h = scaled(a->H, c.volume_scale[i]);
        L.w = scaled(a->W, c.volume_scale[i]);
        REQUIRE(i < 3, "forward: level %d has no feature map (FeatureNet has three scales)", i);
        L.C = fd.c[i]; L.Hs = fd.h[i]; L.Ws = fd.w[i];
        REQUIRE(!(i == 2 && P->tex2), "forward: level_2 texels cannot feed a cost volume");
        REQUIRE(L.D > 0 && L.h > 0 && L.w > 0, "forward: level %d volume is empty", i);
        if (i > 0) REQUIRE(c.depth_inv[i - 1], "forward: cascade levels after a depth-space level are undefined in the "
                                               "reference (utils.py:130)");
        REQUIRE(a->cost_reg_packed[i], "forward: cost_reg_packed[%d] missing", i);
        const long long nv = (long long)a->B * L.D * L.h * L.w;
        L.proj = take((size_t)a->B * a->S * 12);
        L.dv = take((size_t)nv);
        L.nf = take((size_t)a->B * 2 * L.h * L.w);
        L.vol = take((size_t)nv * L.C);
        // only a render samples the level's 8-channel feature volume: where the fused heads can leave it out, an unrendered level
        // neither computes nor holds it (enerf_options_t.heads_keep_feat = 1: the A/B)
        L.prob_only = !c.render_if[i] && !(a->options && a->options->heads_keep_feat) &&
                      cost_reg_feat_optional(resolve_options(a->options), L.C, i != 0, a->B, L.D, L.h, L.w);
        if (!L.prob_only) L.feat3d = take((size_t)nv * 8);
        L.prob = take((size_t)nv);
        L.depth = take((size_t)a->B * L.h * L.w);
        L.std = take((size_t)a->B * L.h * L.w);
        L.dmvs = take((size_t)a->B * L.h * L.w);
        const size_t cw = enerf_cost_reg_workspace_bytes(i != 0, a->B, L.D, L.h, L.w);
        if (cw > P->costreg_ws_bytes) P->costreg_ws_bytes = cw;
        L.render = c.render_if[i] != 0;
        if (!L.render) continue;
        L.Hr = scaled(a->H, c.render_scale[i]);
        L.Wr = scaled(a->W, c.render_scale[i]);
        L.Ns = c.num_samples[i];
        L.F = c.nerf_model_feat_ch[i] + 3;
        REQUIRE(L.Hr > 1 && L.Wr > 1, "forward: level %d render extent too small", i);
        REQUIRE(a->nerf_packed[i], "forward: nerf_packed[%d] missing", i);
        REQUIRE(a->rgb[i] && a->depth[i] && a->weights[i] && a->depth_mvs[i] && a->std[i], "forward: level %d output missing", i);
        const int rc = check_render_feat("forward", c, i, fd, L.Hr, L.Wr, P->hip_feats);
        if (rc != ENERF_OK) return rc;
        L.fl = c.render_im_feat_level[i];
        L.from_l2 = renders_from_l2(c, i, P->tex2);
        if (!P->hip_feats) {
            const double up = c.render_scale[i] / c.im_ibr_scale[i];
            REQUIRE(scaled(fd.h[L.fl], up) == L.Hr && scaled(fd.w[L.fl], up) == L.Wr,
                    "forward: im_feat resolution inconsistent with render_scale / im_ibr_scale at level %d", i);
        }
        if (!L.from_l2) L.tex = take((size_t)n_img * L.Hr * L.Wr * tex_stride(L.F));
        if (a->rays[i] != nullptr) {
            REQUIRE(a->n_rays[i] >= 0, "forward: n_rays[%d] negative", i);
            L.n_rays = a->n_rays[i];
        } else {
            L.n_rays = (long long)L.Hr * L.Wr;
            L.rays = take((size_t)a->B * L.n_rays * 8);
        }
        L.masked = a->mask_at_box != nullptr && i == c.num - 1;
        if (L.masked) {
            REQUIRE(a->B == 1, "forward: mask_at_box needs B == 1 (network_human.py:91 reshapes the mask to (1,-1))");
            REQUIRE(L.n_rays == (long long)a->H * a->W, "forward: mask_at_box has H*W=%lld elements but level %d has %lld rays",
                    (long long)a->H * a->W, i, L.n_rays);
            REQUIRE(a->mask_elem_bytes == 1 || a->mask_elem_bytes == 2 || a->mask_elem_bytes == 4 || a->mask_elem_bytes == 8,
                    "forward: mask_elem_bytes=%d unsupported", a->mask_elem_bytes);
            REQUIRE((a->ray_index != nullptr) == (a->ray_count != nullptr), "forward: pass both ray_index and ray_count or neither");
            REQUIRE(!a->ray_index_ready || a->ray_index, "forward: ray_index_ready without ray_index");
            if (!a->ray_index) { P->ray_index = take((size_t)L.n_rays); P->ray_count = take(64); }
            if (!a->ray_index_ready) P->mask_ws = take(mask_compact_workspace_bytes(L.n_rays) / sizeof(int) + 1);
        }
    }
    P->costreg_ws = take(P->costreg_ws_bytes / sizeof(float));
    P->total_floats = off;
    return ENERF_OK;
}

// what the host can see of a cache against the frame / cascade it is used with (enerf_forward_cached, enerf_source_cache_build)
int check_cache(const char* what, const enerf_source_cache_t* k, const enerf_cascade_t& c, int H, int W) {
    REQUIRE(k, "%s: null cache", what);
    REQUIRE(k->V >= 1, "%s: cache has V=%d views", what, k->V);
    REQUIRE(k->H == H && k->W == W, "%s: cache was built for %dx%d images, the frame has %dx%d", what, k->H, k->W, H, W);
    const int tex2 = cascade_tex2(c);
    REQUIRE(k->l2_stride == l2_stride(tex2), "%s: cache has l2_stride=%d, this cascade needs %d (a cache is valid for the cascade it was built for)",
            what, k->l2_stride, l2_stride(tex2));
    REQUIRE(k->feat_l0 && k->feat_l1 && k->feat_l2 && k->exts && k->ixts, "%s: null cache buffer", what);
    size_t bits = (size_t)k->feat_l0 | (size_t)k->feat_l1 | (size_t)k->feat_l2 | (size_t)k->exts | (size_t)k->ixts;
    for (int i = 0; i < c.num && i < ENERF_MAX_LEVELS; ++i) {
        if (!c.render_if[i] || renders_from_l2(c, i, tex2)) continue;
        REQUIRE(k->tex[i], "%s: cache has no texel image for rendered level %d", what, i);
        bits |= (size_t)k->tex[i];
    }
    REQUIRE((bits & 15) == 0, "%s: cache buffers must be 16-byte aligned", what);
    return ENERF_OK;
}

// =====================================================================================================================
// The frame driver behind enerf_forward (cache == nullptr) and enerf_forward_cached: one FrameRun on the stack per call, one
// member function per stage, run_frame (below) is their sequence.  Stages enqueue on the caller's stream `st` unless they say
// otherwise; the fork/join vocabulary is side_lane.h's record / wait, and need_level(l) is the join in front of the first
// consumer of feature level l on the caller's stream.  Every stage returns ENERF_OK or an error code; after an error run_frame
// leaves through bail(), which joins whatever was forked.
// =====================================================================================================================
// A forked render is a leaf that shares the device with the next level.  As one persistent block per compute unit (130 KB of
// LDS each at C = 32) it kept the next level's LDS-staged kernels off every CU until its blocks exited; on HALF of the CUs,
// with the balanced tile deal, the next level starts at once and the leaf ends under its small layers: lego 543 -> 558
// frames/s (64 blocks 509, 96: 556, 128: 558, 160: 546, all 256: 535; profiles/r06_ab_bg_render_blocks.txt)
constexpr int kBgRenderDiv = 2;          // a forked render's persistent blocks = compute units / this

struct FrameRun {
    const enerf_frame_args_t* a = nullptr;
    const enerf_source_cache_t* cache = nullptr;     // cached frame: the maps, texels and cameras come from here
    const int* view_idx = nullptr;
    FramePlan P;
    hipStream_t st = nullptr;            // the caller's stream
    hipStream_t cur = nullptr;           // the stream the current stage is enqueued on (the lane's for a forked render)
    float* ws = nullptr;
    int n_img = 0;
    float* f[3] = {nullptr, nullptr, nullptr};       // the feature maps, channels-last
    const float *src_exts = nullptr, *src_ixts = nullptr;   // the batch's, or (cached frame) the rows the gather leaves in the workspace
    int *ray_index = nullptr, *ray_count = nullptr;
    // ---- side lane ----
    SideLane* lane = nullptr;
    std::unique_lock<std::mutex> lane_busy;          // held until this call has enqueued its last join (side_lane.h)
    bool forked = false;                 // the sources' later half runs on the side stream
    int joined[3] = {1, 1, 1};           // feature level l is visible to the caller's stream
    int gate_mode = 1;                   // see enerf_options_t.side_gate (resolved by featnet_gate)
    bool stage2_enqueued = true;         // the FeatureNet's last stage (smooth0) has been enqueued (false while gated)
    int stage2_rc = ENERF_OK;
    int render_forks = 0;                // renders of non-final levels enqueued on the lane's render stream
    // ---- the camera-only preparation riding in the frame's first launch (prep_job.h) ----
    PrepJob job;
    int prep_carried = 0;                // a kernel took the job (the fused conv0 pair); otherwise the level loop launches the prep kernels
    // ---- hand-off from level i - 1 to level i ----
    const float *pdepth = nullptr, *pstd = nullptr, *pnf = nullptr;
    int hp = 0, wp = 0;
    const float *pending_prob = nullptr, *pending_dv = nullptr;    // a depth regression deferred into the next level's prep
    int pending_D = 0, pending_inv = 0;
    // ---- inside level i ----
    int vol_planar = 0;                  // the volume goes to conv0 as channel-quad planes
    hipStream_t rs = nullptr;            // the stream of the level's texel / ray / render stages
    bool render_forked = false;
    const float *tex = nullptr, *rays8 = nullptr;

    const enerf_cascade_t& cas() const { return a->cas; }
    bool single_stream() const { return a->options && a->options->single_stream; }
    float* std_of(int i) const { return P.L[i].render ? a->std[i] : ws + P.L[i].std; }

    void mark(int slot) {
#ifndef ENERF_EMU
        if (a->stage_events != nullptr && a->stage_events[slot] != nullptr) hipEventRecord((hipEvent_t)a->stage_events[slot], cur);
#else
        (void)slot;
#endif
    }
    bool take_lane() {                   // this caller stream's lane, locked for the rest of the call; false = one stream
        if (!single_stream()) lane = side_lane(st);
        if (lane != nullptr) lane_busy = std::unique_lock<std::mutex>(lane->busy);
        return lane != nullptr;
    }
    void need_level(int l) {             // call before the first consumer of f[l] on the caller's stream
        if (forked && !joined[l]) { lane->wait(kLaneMain, l == 1 ? kEvL1 : kEvL2); joined[l] = 1; }
    }
    int bail(int code) {                 // error exit: never leave a lane stream un-joined
        if (render_forks > 0) { lane->record(kEvDone, kLaneRender); lane->wait(kLaneMain, kEvDone); }
        need_level(1); need_level(2);
        return code;
    }
    int finish() {
        if (render_forks > 0) lane->wait(kLaneMain, kEvDone);        // join the forked renders
        need_level(1); need_level(2);    // the caller's stream never returns ahead of the side lane
        return check_launch("forward");
    }

    // the plan, and everything the host can refuse before the first launch
    int begin(const enerf_frame_args_t* args, const enerf_source_cache_t* k, const int* idx, enerf_stream_t stream) {
        a = args; cache = k; view_idx = idx;
        int rc = make_plan(a, &P, cache != nullptr);
        if (rc != ENERF_OK) return rc;
        if (cache != nullptr) {
            rc = check_cache("forward_cached", cache, a->cas, a->H, a->W);
            if (rc != ENERF_OK) return rc;
            REQUIRE(view_idx, "forward_cached: null view_idx (a (B,S) int32 device array)");
        }
        REQUIRE(a->workspace, "forward: null workspace");
        if (a->workspace_bytes < P.total_floats * sizeof(float))
            return fail(ENERF_EWORKSPACE, "forward: workspace too small (%zu < %zu bytes)", a->workspace_bytes,
                        P.total_floats * sizeof(float));
        st = cur = rs = (hipStream_t)stream;
        ws = (float*)a->workspace;
        n_img = a->B * a->S;
        for (int l = 0; l < 3; ++l) f[l] = ws + P.f[l];
        src_exts = cache ? ws + P.cam_exts : a->src_exts;
        src_ixts = cache ? ws + P.cam_ixts : a->src_ixts;
        return ENERF_OK;
    }

    // a caller-independent early start for the mask compaction: it only depends on the batch
    void start_mask_compaction() {
        const LevelPlan& last = P.L[cas().num - 1];
        ray_index = a->ray_index; ray_count = a->ray_count;
        if (!(last.render && last.masked)) return;
        if (!ray_index) { ray_index = (int*)(ws + P.ray_index); ray_count = (int*)(ws + P.ray_count); }
        if (!a->ray_index_ready)
            launch_mask_compact(a->mask_at_box, a->mask_elem_bytes, last.n_rays, ray_index, ray_count, ws + P.mask_ws, st);
    }

    // The camera-only preparation — level 0's depth planes and EVERY level's projection matrices (utils.py:35-55, 98-111) — rides
    // in the frame's first launch (prep_job.h): its blocks run beside conv0's instead of as a launch of their own between the trunk
    // and the warp.  Only the HIP FeatureNet has that launch: the NCHW and cached frames keep the level loop's own prep launches (a
    // cached frame's preparation reads the GATHERED camera rows).
    void make_prep_job() {
        memset(&job, 0, sizeof(job));
        if (!P.hip_feats || cache != nullptr) return;
        const enerf_cascade_t& c = cas();
        const LevelPlan& L0 = P.L[0];
        job.near_far = a->near_far; job.dv = ws + L0.dv; job.nf = ws + L0.nf;
        job.B = a->B; job.D = L0.D; job.h = L0.h; job.w = L0.w; job.depth_inv = c.depth_inv[0];
        for (int i = 0; i < c.num && i < 3; ++i)
            job.pj[i] = ProjJob{a->src_ixts, a->src_exts, a->tar_ixt, a->tar_ext, ws + P.L[i].proj, a->S, (float)c.im_feat_scale[i],
                                (float)c.volume_scale[i]};
        job.nblocks = prep_job_blocks(a->B, L0.D, L0.h, L0.w, 256);
    }

    // ---- sources, cached frame: gather the selected views' maps, texels and cameras instead of computing them.  Level 0 / level 1
    // maps, the non-final levels' texels and the cameras (everything the chain needs first) on the caller's stream; the level-2 map
    // and the last level's texels, two thirds of the bytes and needed only by the final render, on the side stream.
    int sources_cached() {
        const enerf_cascade_t& c = cas();
        const FeatDims fd(a->H, a->W);
        GatherJob main_job, side_job;
        memset(&main_job, 0, sizeof(main_job));
        memset(&side_job, 0, sizeof(side_job));
        main_job.V = side_job.V = cache->V;
        main_job.view_idx = side_job.view_idx = view_idx;
        main_job.exts = cache->exts; main_job.ixts = cache->ixts;
        main_job.dst_exts = ws + P.cam_exts; main_job.dst_ixts = ws + P.cam_ixts;
        auto add = [](GatherJob& J, const float* src, float* dst, long long floats_per_view) {
            J.seg[J.nseg++] = GatherSeg{reinterpret_cast<const float4*>(src), reinterpret_cast<float4*>(dst), floats_per_view / 4};
        };
        add(main_job, cache->feat_l0, f[0], fd.pixels(0) * fd.c[0]);
        add(main_job, cache->feat_l1, f[1], fd.pixels(1) * fd.c[1]);
        bool uses2 = c.num >= 3;                      // level_2 feeds a third level's cost volume, or IS a render's texels (stride 12);
        for (int i = 0; i < c.num; ++i)               // a render from the plain map reads its own texel image instead
            uses2 = uses2 || P.L[i].from_l2;
        if (uses2) add(side_job, cache->feat_l2, f[2], fd.pixels(2) * cache->l2_stride);
        for (int i = 0; i < c.num; ++i) {
            const LevelPlan& L = P.L[i];
            if (!L.render || L.from_l2) continue;
            add(i + 1 < c.num ? main_job : side_job, cache->tex[i], ws + L.tex, (long long)L.Hr * L.Wr * tex_stride(L.F));
        }
        if (side_job.nseg > 0 && take_lane()) {
            lane->record(kEvTrunk, kLaneMain);         // the lane starts behind the previous frame and the producer of view_idx
            lane->wait(kLaneSide, kEvTrunk);
            launch_gather_sources(main_job, n_img, st);
            launch_gather_sources(side_job, n_img, lane->stream[kLaneSide]);
            lane->record(kEvL1, kLaneSide);
            lane->record(kEvL2, kLaneSide);
            forked = true; joined[1] = 1; joined[2] = 0;       // (level 1 came with the caller's stream)
        } else {
            for (int s = 0; s < side_job.nseg; ++s) main_job.seg[main_job.nseg++] = side_job.seg[s];
            launch_gather_sources(main_job, n_img, st);
        }
        return check_launch("forward_cached: gather");
    }

    // ---- sources, HIP FeatureNet (feature_net.py:27-36) -> channels-last maps; level_2 straight to render texels when it can.
    // With a lane: the trunk on the caller's stream, the top-down half forked behind it.
    int featnet_stage(int stage, hipStream_t s) {
        const bool first = stage == ENERF_FEAT_ALL || stage == ENERF_FEAT_TRUNK;
        return feature_net_stage_job(a->feature_net_packed, a->src_inps, n_img, a->H, a->W, f[0], f[1], f[2], l2_stride(P.tex2),
                                     ws + P.featnet_ws, P.featnet_ws_bytes, stage, a->options, s,
                                     first && job.nblocks > 0 ? &job : nullptr, first ? &prep_carried : nullptr);
    }
    // The last stage (lat0 + smooth0 -> render texels) is needed only by the final render.  Enqueued with the fork (default) it
    // shares the chip with level 0; GATED (enerf_options_t.side_gate >= 2) it is enqueued later, from inside the last level's cost
    // regularisation, behind an event, to run beside that level's small deep layers instead.  Measured in round 3
    // (profiles/r03_ab_side_gate.txt): gating LOSES 1-2 % on all three workloads — the early start wins.
    void featnet_gate() {
        const enerf_cascade_t& c = cas();
        gate_mode = a->options ? a->options->side_gate : 0;
        if (gate_mode == 0) gate_mode = 1;
        const int lastl = c.num - 1;
        const bool gateable = c.num >= 2 && P.tex2 && c.render_if[lastl] && c.render_im_feat_level[lastl] == 2;
        for (int l = 0; l < lastl && gateable; ++l)                       // nobody before the last level may need level_2
            if (c.render_if[l] && c.render_im_feat_level[l] == 2) gate_mode = 1;
        if (!gateable) gate_mode = 1;
    }
    int sources_featnet() {
        if (!take_lane()) return featnet_stage(ENERF_FEAT_ALL, st);
        int rc = featnet_stage(ENERF_FEAT_TRUNK, st);
        if (rc != ENERF_OK) return rc;
        lane->record(kEvTrunk, kLaneMain);
        lane->wait(kLaneSide, kEvTrunk);
        rc = featnet_stage(ENERF_FEAT_LEVEL1, lane->stream[kLaneSide]);
        lane->record(kEvL1, kLaneSide);
        featnet_gate();
        if (gate_mode == 1) {
            if (rc == ENERF_OK) rc = featnet_stage(ENERF_FEAT_LEVEL2, lane->stream[kLaneSide]);
            lane->record(kEvL2, kLaneSide);
        } else
            stage2_enqueued = false;         // level_cost_reg of the last level enqueues it
        forked = true; joined[1] = joined[2] = 0;
        return rc;
    }
    // deferred enqueue of the FeatureNet's last stage on the side stream, behind an event recorded on the caller's stream NOW
    void enqueue_stage2() {
        if (stage2_enqueued || lane == nullptr) return;
        lane->record(kEvFork, kLaneMain);                                 // "the chain has reached this point"
        lane->wait(kLaneSide, kEvFork);
        stage2_rc = featnet_stage(ENERF_FEAT_LEVEL2, lane->stream[kLaneSide]);
        lane->record(kEvL2, kLaneSide);
        stage2_enqueued = true;
    }

    // ---- sources, NCHW maps from torch: the levels that feed a cost volume (texels are packed from NCHW in level_texels) ----
    int sources_nchw() {
        const FeatDims fd(a->H, a->W);
        for (int l = 0; l < cas().num; ++l) launch_channels_last(a->feats_nchw[l], f[l], n_img, fd.c[l], fd.pixels(l), fd.c[l], st);
        return ENERF_OK;
    }

    // ---- level i: projection matrices and depth hypotheses.  The previous level's depth regression rides in this launch when that
    // level is not rendered (its depth / std are then only this level's inputs): one launch instead of two on the critical chain
    // between the levels.
    int level_prep(int i) {
        const enerf_cascade_t& c = cas();
        const LevelPlan& L = P.L[i];
        float *proj = ws + L.proj, *dv = ws + L.dv, *nf = ws + L.nf;
        bool prep_done = false;
        if (pending_prob != nullptr) {
            // (the level's projection matrices are already there when the frame's first launch carried the preparation job)
            prep_done = launch_regress_and_values(src_ixts, src_exts, a->tar_ixt, a->tar_ext, a->S, (float)c.im_feat_scale[i],
                                                  (float)c.volume_scale[i], prep_carried && i < 3 ? nullptr : proj, pending_prob, pending_dv, pnf, pending_D, hp, wp,
                                                  pending_inv, const_cast<float*>(pdepth), const_cast<float*>(pstd), a->B, L.D,
                                                  L.h, L.w, c.depth_inv[i], dv, nf, st);
            if (!prep_done)         // shape outside the fused kernel's limits: the two separate launches
                launch_depth_regression(pending_prob, pending_dv, a->B, pending_D, hp, wp, pending_inv,
                                        const_cast<float*>(pdepth), const_cast<float*>(pstd), nullptr, st);
            pending_prob = nullptr;
        }
        if (i == 0 && prep_carried) prep_done = true;                  // level 0: planes + matrices came with the first launch
        int rc;
        if (!prep_done)
            rc = enerf_level_prep(src_ixts, src_exts, a->tar_ixt, a->tar_ext, a->B, a->S, (float)c.im_feat_scale[i],
                                  (float)c.volume_scale[i], proj, a->near_far, pdepth, pstd, pnf, L.D, L.h, L.w, hp, wp,
                                  c.depth_inv[i], dv, nf, st);
        else
            rc = check_launch("level_prep");
        if (rc == ENERF_OK) mark(ENERF_STAGE_LEVEL(i, ENERF_STAGE_PREP));
        return rc;
    }

    // ---- level i: the warped feature volume, as channel-quad planes when conv0 runs on the asynchronously staged kernel ----
    int level_volume(int i) {
        const LevelPlan& L = P.L[i];
        float *proj = ws + L.proj, *dv = ws + L.dv, *vol = ws + L.vol;
        need_level(i);                                                     // level i's source maps (side stream for i >= 1)
        vol_planar = cost_reg_conv0_planar(resolve_options(a->options), L.C, i != 0, a->B, L.D, L.h, L.w) ? 1 : 0;
        int rc;
        if (!vol_planar)
            rc = enerf_build_feature_volume(f[i], proj, dv, a->B, a->S, L.C, L.Hs, L.Ws, L.D, L.h, L.w, vol, st);
        else {      // same argument checks as the C entry (shapes come from the validated plan; the 32-bit limits are re-checked)
            REQUIRE((long long)a->B * a->S * L.Hs * L.Ws * L.C < (1LL << 32) && (long long)L.Hs * L.Ws < (1LL << 23) &&
                    (long long)a->B * L.D * L.h * L.w * (L.C / 4) < (1LL << 31) && (long long)L.h * L.w < (1LL << 23) &&
                    (long long)a->B * L.D <= 65535 && (long long)a->B * L.D * L.h < (1LL << 23) && L.w < (1 << 23),
                    "forward: level %d volume too large for 32-bit indices / the grid-carried voxel decomposition", i);
            launch_feature_volume(f[i], proj, dv, a->B, a->S, L.C, L.Hs, L.Ws, L.D, L.h, L.w, vol, st, 1);
            rc = check_launch("build_feature_volume");
        }
        if (rc == ENERF_OK) mark(ENERF_STAGE_LEVEL(i, ENERF_STAGE_VOLUME));
        return rc;
    }

    // ---- level i: CostRegNet.  On the last level a gated FeatureNet stage 2 is enqueued around it: before it (side_gate 3), from
    // its hook after conv0 (2) or conv2 (4), and in any case behind it (an error path inside cost_reg skips the hook).
    int level_cost_reg(int i) {
        const LevelPlan& L = P.L[i];
        const CostRegHook hook = {[](void* self) { static_cast<FrameRun*>(self)->enqueue_stage2(); }, this, gate_mode == 4 ? 2 : 0};
        const CostRegHook* hk = nullptr;
        const bool gated_here = !stage2_enqueued && i == cas().num - 1;
        if (gated_here) {
            if (gate_mode == 3) enqueue_stage2(); else hk = &hook;
        }
        int rc = cost_reg_run(a->cost_reg_packed[i], L.C, i != 0, ws + L.vol, vol_planar, a->B, L.D, L.h, L.w,
                              L.prob_only ? nullptr : ws + L.feat3d, ws + L.prob, ws + P.costreg_ws, P.costreg_ws_bytes, a->options, st, hk);
        if (gated_here) enqueue_stage2();
        if (rc == ENERF_OK && stage2_rc != ENERF_OK) rc = stage2_rc;
        if (rc == ENERF_OK) mark(ENERF_STAGE_LEVEL(i, ENERF_STAGE_COST_REG));
        return rc;
    }

    // ---- level i: depth regression — now, or (level not rendered, a next level follows) deferred into that level's prep launch;
    // then the hand-off to level i + 1
    int level_depth(int i) {
        const enerf_cascade_t& c = cas();
        const LevelPlan& L = P.L[i];
        float *prob = ws + L.prob, *dv = ws + L.dv, *depth = ws + L.depth, *std = std_of(i);
        const bool defer_regression = !L.render && i + 1 < c.num && !(a->options && a->options->fuse_depth_prep == 1);
        if (defer_regression) { pending_prob = prob; pending_dv = dv; pending_D = L.D; pending_inv = c.depth_inv[i]; }
        else launch_depth_regression(prob, dv, a->B, L.D, L.h, L.w, c.depth_inv[i], depth, std, L.render ? a->depth_mvs[i] : nullptr, st);
        mark(ENERF_STAGE_LEVEL(i, ENERF_STAGE_DEPTH_REG));
        pdepth = depth; pstd = std; pnf = ws + L.nf; hp = L.h; wp = L.w;
        return ENERF_OK;
    }

    // ---- rendered level i, texels: unpreprocess + cat (network.py:28-34) as the channels-last gather source.  The texel source is
    // joined here; a non-final level's render is a leaf of the frame, so its three stages are forked onto the render stream (its
    // inputs are complete on the caller's stream here).
    int level_texels(int i) {
        const enerf_cascade_t& c = cas();
        const LevelPlan& L = P.L[i];
        const FeatDims fd(a->H, a->W);
        const int fl = L.fl, TEX = tex_stride(L.F);
        if (cache == nullptr || L.from_l2) need_level(fl);
        rs = st; render_forked = false;
        if (forked && i + 1 < c.num && !L.masked) {
            if (render_forks > 0) lane->wait(kLaneRender, kEvDone);       // (ordering only: same stream anyway)
            lane->record(kEvFork, kLaneMain);
            lane->wait(kLaneRender, kEvFork);
            rs = cur = lane->stream[kLaneRender]; render_forked = true; ++render_forks;
        }
        int rc = ENERF_OK;
        if (L.from_l2) tex = f[2];
        else if (cache != nullptr) {                                       // gathered with the maps; the last level's on the side stream
            if (i + 1 == c.num) need_level(2);
            tex = ws + L.tex;
        } else {
            float* t = ws + L.tex;
            if (P.hip_feats)
                rc = enerf_pack_texels_cl(f[fl], fd.c[fl], a->src_inps, a->H, a->W, L.Hr, L.Wr, TEX, n_img, t, rs);
            else
                rc = enerf_pack_img_feat_rgb(a->feats_nchw[fl], fd.c[fl], fd.h[fl], fd.w[fl], a->src_inps, a->H, a->W, L.Hr, L.Wr,
                                             TEX, n_img, t, rs);
            tex = t;
        }
        if (rc == ENERF_OK) mark(ENERF_STAGE_LEVEL(i, ENERF_STAGE_TEXELS));
        return rc;
    }

    // ---- rendered level i, rays: the batch's, or the full image generated here (enerf_utils.py:61-71) ----
    int level_rays(int i) {
        const LevelPlan& L = P.L[i];
        rays8 = a->rays[i];
        if (rays8 != nullptr) return ENERF_OK;
        float* r = ws + L.rays;
        rays8 = r;
        return enerf_gen_rays(a->tar_ext, a->tar_ixt, a->B, L.Hr, L.Wr, (float)cas().render_scale[i], r, rs);
    }

    // ---- rendered level i: build_rays + render_rays (utils.py:390-420, network.py:24-43), one launch ----
    int level_render(int i) {
        const enerf_cascade_t& c = cas();
        const LevelPlan& L = P.L[i];
        enerf_render_args_t ra;
        memset(&ra, 0, sizeof(ra));
        ra.tex = tex; ra.vol = ws + L.feat3d; ra.src_exts = src_exts; ra.src_ixts = src_ixts; ra.tar_ext = a->tar_ext;
        ra.packed = a->nerf_packed[i];
        ra.rgb = a->rgb[i]; ra.depth = a->depth[i]; ra.weights = a->weights[i];
        ra.B = a->B; ra.N = (int)L.n_rays; ra.S = a->S; ra.n_samples = L.Ns; ra.depth_inv = c.depth_inv[i];
        ra.Hr = L.Hr; ra.Wr = L.Wr; ra.F = L.F; ra.D = L.D; ra.h = L.h; ra.w = L.w; ra.white_bkgd = c.white_bkgd;
        ra.render_scale = (float)c.render_scale[i];
        ra.rays8 = rays8; ra.depth_map = ws + L.depth; ra.std_map = std_of(i); ra.nf_map = ws + L.nf; ra.map_h = L.h; ra.map_w = L.w;
        ra.options = a->options;
        if (render_forked) ra.max_blocks = device_cu_count() / kBgRenderDiv;
        if (L.masked) {
            ra.ray_index = ray_index; ra.ray_count = ray_count; ra.scatter_rgb = 1;
            zero_async(a->rgb[i], (size_t)L.n_rays * 3 * sizeof(float), rs);      // torch.zeros_like(...), network_human.py:103
        }
        const int rc = enerf_render_rays(&ra, rs);
        if (rc != ENERF_OK) return rc;
        mark(ENERF_STAGE_LEVEL(i, ENERF_STAGE_RENDER));
        if (render_forked) { lane->record(kEvDone, kLaneRender); cur = st; }
        return ENERF_OK;
    }
};

int run_frame(const enerf_frame_args_t* a, const enerf_source_cache_t* cache, const int* view_idx, enerf_stream_t stream) {
    FrameRun R;
    int rc = R.begin(a, cache, view_idx, stream);
    if (rc != ENERF_OK) return rc;
    R.mark(ENERF_STAGE_BEGIN);
    R.start_mask_compaction();
    R.make_prep_job();
    rc = cache != nullptr ? R.sources_cached() : R.P.hip_feats ? R.sources_featnet() : R.sources_nchw();
    if (rc != ENERF_OK) return R.bail(rc);
    R.mark(ENERF_STAGE_FEATURE_NET);
    for (int i = 0; i < a->cas.num; ++i) {
        rc = R.level_prep(i);
        if (rc == ENERF_OK) rc = R.level_volume(i);
        if (rc == ENERF_OK) rc = R.level_cost_reg(i);
        if (rc == ENERF_OK) rc = R.level_depth(i);
        if (rc == ENERF_OK && R.P.L[i].render) {
            rc = R.level_texels(i);
            if (rc == ENERF_OK) rc = R.level_rays(i);
            if (rc == ENERF_OK) rc = R.level_render(i);
        }
        if (rc != ENERF_OK) return R.bail(rc);
    }
    return R.finish();
}

// =====================================================================================================================
// The composite network's frame (enerf_forward_composite; network_composite.py:77-146): L boxed foreground cascades over one
// background cascade, merged per rendered level by enerf_composite_layers.  Same shape as the driver above — a plan that refuses
// everything the host can see and carves the workspace, one CompositeRun on the stack with one member function per stage,
// run_composite their sequence — but the stages are the library's separate C entries, called exactly as a host stitching the
// frame together itself would call them (the windowed volume and regression for a layer, cost_reg on a channels-last volume, the
// raw render without a voxel volume), so the frame's bits are that host's bits.  Only the camera-only preparation differs: one
// k_composite_prep launch at the head of the frame instead of a launch per level, cascade and window.
//
// Streams (side_lane.h): cascade L (the background) and feature_net_bg stay on the caller's stream; feature_net, the texel packs of
// src_inps and layer l's cascade + raw renders go to `side` (even l) or `render` (odd l), forked behind the preparation and
// joined in front of every rendered level's merge and at every exit.
//
// Workspace regions by chain — chains may overlap in time, so no region has two owners:
//   shared, written before the fork (prep launch, ray generation on the caller's stream), read-only after: every level's proj and
//           rays, level 0's dv / nf of every cascade, every window's ray index / count;
//   foreground sources (`side`): f_fg[0..2], featws_fg, tex_fg of every rendered level — read-only for the layers after `feats`;
//   layer l (its lane stream): C[i][l].{dv, nf (i > 0), vol, feat3d, prob, depth, std, raw, z} of every level i, costreg_ws[l];
//   background (caller's stream): f_bg[0..2], featws_bg, tex_bg, C[i][L].*, costreg_ws[L].
// A layer's raw / z and the caller's outputs meet only in enerf_composite_layers, behind the join.
//
// A cached frame (enerf_forward_composite_cached; `cached` below) takes both nets' maps, the texels and the source cameras from an
// enerf_composite_cache_t behind a device-side view index: the preparation launch reads its cameras through the index and leaves the
// gathered rows in cam_exts / cam_ixts and the "an index was outside the cache" flag the merges read in `invalid` (shared: written
// before the fork, read-only after), and the sources are two k_gather_sources
// launches into the regions the FeatureNets and texel packs wrote — the foreground's on `side`, the background's on the caller's
// stream, same owners as above.  No FeatureNet scratch, and no region for a feature map that no cost volume reads.
// =====================================================================================================================
constexpr int kCompCascades = ENERF_MAX_FG_LAYERS + 1;
struct CompLevel {
    int h, w, C, Hs, Ws, inv;              // volume grid, cost-volume channels, source-map size, depth_inv
    int Hr, Wr, render, F, Ns, fl;         // render raster, flag, nerf feature width, samples per ray, texel feature level
    int vwin[ENERF_MAX_FG_LAYERS][4];      // layer windows (x0, y0, ww, wh) of the volume grid ...
    int rwin[ENERF_MAX_FG_LAYERS][4];      // ... and of the render raster
    size_t proj, rays, tex_fg, tex_bg;
};
struct CompCascadeLevel {
    int D, wh, ww, rows;                   // planes; the cost volume's extent (the window, or the grid); raw-render rows
    size_t dv, nf, vol, feat3d, prob, depth, std, raw, z, index, count;
    size_t costreg_bytes;
};
struct CompositePlan {
    size_t f_fg[3], f_bg[3], featws_fg, featws_bg, featws_bytes;
    size_t cam_exts, cam_ixts, invalid;    // cached frame: the gathered (1,S,4,4) / (1,S,3,3) camera rows; "an index was outside the cache"
    size_t wintab;                         // moving boxes: the windows' resolved corners (kWinTableInts ints), then the L flags
    int bw[ENERF_MAX_FG_LAYERS], bh[ENERF_MAX_FG_LAYERS];     // moving boxes: the layers' sizes in input-image pixels
    CompLevel L[ENERF_MAX_LEVELS];
    CompCascadeLevel C[ENERF_MAX_LEVELS][kCompCascades];
    size_t costreg_ws[kCompCascades], costreg_ws_bytes[kCompCascades];
    size_t total_floats;
};
// (bbox * scale).int() of network_composite.py:88 / utils.py:879: float32 product, truncation
inline void scaled_box(const float* box, double scale, int* win) {
    const float sc = (float)scale;
    for (int k = 0; k < 4; ++k) { const volatile float v = box[k] * sc; win[k] = (int)v; }
}
int check_comp_window(const char* grid, int level, int l, const int* wn, int h, int w) {
    REQUIRE(wn[2] > 0 && wn[3] > 0 && wn[0] >= 0 && wn[1] >= 0 && (long long)wn[0] + wn[2] <= w && (long long)wn[1] + wn[3] <= h,
            "forward_composite: bbox[%d] at level %d is the window (x0 %d, y0 %d, %d x %d), outside the %d x %d %s", l, level, wn[0], wn[1],
            wn[2], wn[3], w, h, grid);
    return ENERF_OK;
}

// `moving` (enerf_forward_composite_moving): the plan depends on the boxes' sizes alone — every window is laid out, and refused, as
// the box (0, 0, w, h), a box larger than the image is refused, and the workspace gets the table of the corners the preparation
// launch resolves from the positions on the device.
int make_composite_plan(const enerf_composite_frame_args_t* a, CompositePlan* P, bool cached = false, bool moving = false) {
    REQUIRE(a, "forward_composite: null args");
    const enerf_cascade_t& c = a->cas;
    const int L = a->L;
    REQUIRE(L >= 1 && L <= ENERF_MAX_FG_LAYERS, "forward_composite: L=%d foreground layers unsupported (1..%d)", L, ENERF_MAX_FG_LAYERS);
    REQUIRE(c.num >= 1 && c.num <= ENERF_MAX_LEVELS, "forward_composite: cas.num=%d unsupported (1..%d)", c.num, ENERF_MAX_LEVELS);
    REQUIRE(a->S >= 2 && a->S <= 4 && a->H > 0 && a->W > 0 && a->H % 4 == 0 && a->W % 4 == 0,
            "forward_composite: bad frame shape S=%d H=%d W=%d (S in 2..4, H and W divisible by 4)", a->S, a->H, a->W);
    if (!cached) {                         // (a cached frame takes these from the cache)
        REQUIRE(a->src_inps && a->bg_src_inps, "forward_composite: src_inps / bg_src_inps is null");
        REQUIRE(a->src_exts && a->src_ixts && a->tar_ext && a->tar_ixt, "forward_composite: src_exts / src_ixts / tar_ext / tar_ixt is null");
    } else
        REQUIRE(a->tar_ext && a->tar_ixt, "forward_composite: tar_ext / tar_ixt is null");
    REQUIRE(a->near_far, "forward_composite: near_far is null");
    if (!cached)
        REQUIRE(a->feature_net_packed && a->feature_net_bg_packed, "forward_composite: feature_net_packed / feature_net_bg_packed is null");
    int covered = 0;
    while (covered < ENERF_MAX_LEVELS && a->bg_volume_planes[covered] > 0) ++covered;
    REQUIRE(c.num <= covered, "forward_composite: cas.num=%d levels but bg_volume_planes covers %d", c.num, covered);
    for (int i = 0; i < c.num; ++i)
        if (c.render_if[i]) {
            REQUIRE(c.num_samples[i] >= 1 && L * c.num_samples[i] <= 16, "forward_composite: L * num_samples = %d * %d at level %d unsupported (at most 16)",
                    L, c.num_samples[i], i);
            REQUIRE(c.num_samples[i] <= 8, "forward_composite: cas.num_samples[%d]=%d unsupported (the render kernel takes 1..8 samples per ray)", i,
                    c.num_samples[i]);
        }
    memset(P, 0, sizeof(*P));
    size_t off = 0;
    auto take = [&](size_t nfloats) { size_t r = off; off += (nfloats + 63) / 64 * 64; return r; };   // 256-B aligned
    const FeatDims fd(a->H, a->W);
    const int S = a->S;
    if (!cached) {
        for (int l = 0; l < 3; ++l) P->f_fg[l] = take((size_t)S * fd.pixels(l) * fd.c[l]);
        for (int l = 0; l < 3; ++l) P->f_bg[l] = take((size_t)S * fd.pixels(l) * fd.c[l]);
        P->featws_bytes = enerf_feature_net_workspace_bytes(S, a->H, a->W);
        P->featws_fg = take(P->featws_bytes / sizeof(float));
        P->featws_bg = take(P->featws_bytes / sizeof(float));
    } else {                               // only the maps a cost volume reads; the cameras' rows instead of the FeatureNets' scratch
        int segs = c.num;
        for (int i = 0; i < c.num; ++i) segs += c.render_if[i] != 0;
        REQUIRE(segs <= kGatherSegs, "forward_composite: cas.num=%d levels with %d rendered need %d gather segments per net (at most %d)",
                c.num, segs - c.num, segs, kGatherSegs);
        for (int l = 0; l < c.num && l < 3; ++l) P->f_fg[l] = take((size_t)S * fd.pixels(l) * fd.c[l]);
        for (int l = 0; l < c.num && l < 3; ++l) P->f_bg[l] = take((size_t)S * fd.pixels(l) * fd.c[l]);
        P->cam_exts = take((size_t)S * 16);
        P->cam_ixts = take((size_t)S * 9);
        P->invalid = take(64);
    }
    if (moving) {
        for (int l = 0; l < L; ++l) {
            const float bw = a->bbox[l][2], bh = a->bbox[l][3];
            REQUIRE(bw >= 1.f && bh >= 1.f && bw <= (float)a->W && bh <= (float)a->H,
                    "forward_composite_moving: bbox[%d] has the size %g x %g (w, h): w > W, h > H or an empty box in a %d x %d image", l, (double)bw,
                    (double)bh, a->W, a->H);
            P->bw[l] = (int)ceilf(bw); P->bh[l] = (int)ceilf(bh);
        }
        P->wintab = take(kWinTableInts + ENERF_MAX_FG_LAYERS);
    }
    for (int i = 0; i < c.num; ++i) {
        CompLevel& V = P->L[i];
        V.h = scaled(a->H, c.volume_scale[i]);
        V.w = scaled(a->W, c.volume_scale[i]);
        V.C = fd.c[i]; V.Hs = fd.h[i]; V.Ws = fd.w[i]; V.inv = c.depth_inv[i];
        REQUIRE(V.C == 16 || V.C == 32, "forward_composite: cas.num: level %d would warp %d-channel features (the windowed volume has 16 / 32)", i, V.C);
        REQUIRE(V.h > 0 && V.w > 0 && V.h % 4 == 0 && V.w % 4 == 0,
                "forward_composite: level %d volume grid h, w (%d, %d) of H, W (%d, %d) must be divisible by 4", i, V.h, V.w, a->H, a->W);
        if (i > 0) REQUIRE(c.depth_inv[i - 1], "forward_composite: cas.depth_inv: cascade levels after a depth-space level are undefined in the "
                                               "reference (utils.py:130)");
        REQUIRE((long long)S * V.Hs * V.Ws * V.C < (1LL << 32) && (long long)V.Hs * V.Ws < (1LL << 23) && (long long)V.h * V.w < (1LL << 23),
                "forward_composite: H, W: level %d too large for 32-bit gather offsets", i);
        V.render = c.render_if[i] != 0;
        V.proj = take((size_t)S * 12);
        if (V.render) {
            V.Hr = scaled(a->H, c.render_scale[i]);
            V.Wr = scaled(a->W, c.render_scale[i]);
            V.Ns = c.num_samples[i];
            V.F = c.nerf_model_feat_ch[i] + 3;
            REQUIRE(V.Hr > 1 && V.Wr > 1, "forward_composite: cas.render_scale: level %d render extent too small", i);
            REQUIRE(V.F == 11 || V.F == 35, "forward_composite: cas.nerf_model_feat_ch[%d]=%d unsupported (8 or 32)", i, V.F - 3);
            REQUIRE((long long)V.Hr * V.Wr * (L + 1) * V.Ns * 4 < (1LL << 31), "forward_composite: H, W: level %d render image too large", i);
            {   // the raw render's own refusals (render.hip), asked here so that none is left for behind the fork
                RenderArgs probe;
                memset(&probe, 0, sizeof(probe));
                probe.B = 1; probe.S = S; probe.N = V.Hr * V.Wr; probe.n_samples = V.Ns; probe.Hr = V.Hr; probe.Wr = V.Wr; probe.F = V.F;
                probe.D = probe.h = probe.w = 1;                   // (vol = NULL: enerf_render_rays_raw passes ones)
                const int code = render_rays_raw_check(probe);
                REQUIRE(code != -5, "forward_composite: H, W: level %d render raster %d x %d with S=%d too large for the render kernel's 32-bit byte offsets",
                        i, V.Wr, V.Hr, S);
                REQUIRE(code == 0, "forward_composite: level %d render configuration unsupported (code %d: nerf_model_feat_ch=%d S=%d num_samples=%d)", i,
                        code, V.F - 3, S, V.Ns);
            }
            if (int rc = check_render_feat("forward_composite", c, i, fd, V.Hr, V.Wr, true)) return rc;
            V.fl = c.render_im_feat_level[i];
            REQUIRE(a->rgb[i] && a->depth[i] && a->weights[i] && a->net_output[i] && a->z_vals[i],
                    "forward_composite: level %d output (rgb / depth / weights / net_output / z_vals) is null", i);
            REQUIRE((uintptr_t)a->net_output[i] % 16 == 0, "forward_composite: net_output[%d] must be 16-byte aligned", i);
            if (a->rays[i] == nullptr) V.rays = take((size_t)V.Hr * V.Wr * 8);
            V.tex_fg = take((size_t)S * V.Hr * V.Wr * tex_stride(V.F));
            V.tex_bg = take((size_t)S * V.Hr * V.Wr * tex_stride(V.F));
        }
        for (int k = 0; k <= L; ++k) {
            CompCascadeLevel& K = P->C[i][k];
            const bool fg = k < L;
            K.D = fg ? c.volume_planes[i] : a->bg_volume_planes[i];
            REQUIRE(K.D > 0 && K.D % 4 == 0 && K.D <= 64, "forward_composite: %s[%d]=%d planes unsupported (divisible by 4, at most 64)",
                    fg ? "cas.volume_planes" : "bg_volume_planes", i, K.D);
            K.wh = V.h; K.ww = V.w; K.rows = V.render ? V.Hr * V.Wr : 0;
            if (fg) {
                const float at_origin[4] = {0.f, 0.f, a->bbox[k][2], a->bbox[k][3]};
                const float* box = moving ? at_origin : a->bbox[k];
                scaled_box(box, c.volume_scale[i], V.vwin[k]);
                if (int rc = check_comp_window("volume grid", i, k, V.vwin[k], V.h, V.w)) return rc;
                K.ww = V.vwin[k][2]; K.wh = V.vwin[k][3];
                REQUIRE(K.ww % 4 == 0 && K.wh % 4 == 0, "forward_composite: bbox[%d] at level %d is a %d x %d window: ww, wh must be divisible by 4",
                        k, i, K.ww, K.wh);
                if (V.render) {
                    scaled_box(box, c.render_scale[i], V.rwin[k]);
                    if (int rc = check_comp_window("ray raster", i, k, V.rwin[k], V.Hr, V.Wr)) return rc;
                    K.rows = V.rwin[k][2] * V.rwin[k][3];
                }
            }
            REQUIRE(a->cost_reg_packed[i][k], "forward_composite: cost_reg_packed[%d][%d] is null", i, k);
            if (V.render) REQUIRE(a->nerf_packed[i][k], "forward_composite: nerf_packed[%d][%d] is null", i, k);
            const size_t grid = (size_t)V.h * V.w, vox = (size_t)K.D * K.wh * K.ww;
            REQUIRE((long long)K.D * V.h * V.w * (V.C / 4) < (1LL << 31) && (long long)K.D * V.h < (1LL << 23),
                    "forward_composite: H, W: level %d volume too large for 32-bit voxel indices", i);
            K.dv = take((size_t)K.D * grid);
            K.nf = take(2 * grid);
            K.vol = take(vox * V.C);
            K.feat3d = take(vox * 8);
            K.prob = take(vox);
            if (a->depth_map[i][k] == nullptr) K.depth = take(grid);
            if (a->std_map[i][k] == nullptr) K.std = take(grid);
            if (V.render) {
                K.raw = take((size_t)K.rows * V.Ns * 4);
                K.z = take((size_t)K.rows * V.Ns);
                if (fg) { K.index = take((size_t)K.rows); K.count = take(64); }
            }
            K.costreg_bytes = enerf_cost_reg_workspace_bytes(0, 1, K.D, K.wh, K.ww);
            if (K.costreg_bytes > P->costreg_ws_bytes[k]) P->costreg_ws_bytes[k] = K.costreg_bytes;
        }
    }
    for (int k = 0; k <= L; ++k) P->costreg_ws[k] = take(P->costreg_ws_bytes[k] / sizeof(float) + 1);
    P->total_floats = off;
    return ENERF_OK;
}

// what the host can see of a composite cache against the frame / cascade it is used with
int check_composite_cache(const char* what, const enerf_composite_cache_t* k, const enerf_cascade_t& c, int H, int W) {
    REQUIRE(k, "%s: null cache", what);
    REQUIRE(k->V >= 1, "%s: cache has V=%d views", what, k->V);
    REQUIRE(k->H == H && k->W == W, "%s: cache was built for %dx%d images (H, W), the frame has %dx%d", what, k->H, k->W, H, W);
    REQUIRE(k->exts && k->ixts, "%s: cache has no exts / ixts", what);
    size_t bits = (size_t)k->exts | (size_t)k->ixts;
    for (int i = 0; i < c.num && i < ENERF_MAX_LEVELS; ++i) {
        REQUIRE(k->fg_feat[i] && k->bg_feat[i], "%s: cache has no %s[%d], the feature map of cascade level %d", what,
                k->fg_feat[i] ? "bg_feat" : "fg_feat", i, i);
        bits |= (size_t)k->fg_feat[i] | (size_t)k->bg_feat[i];
        if (!c.render_if[i]) continue;
        REQUIRE(k->fg_tex[i] && k->bg_tex[i], "%s: cache has no %s[%d], the texel image of rendered level %d", what,
                k->fg_tex[i] ? "bg_tex" : "fg_tex", i, i);
        bits |= (size_t)k->fg_tex[i] | (size_t)k->bg_tex[i];
    }
    REQUIRE((bits & 15) == 0, "%s: cache buffers must be 16-byte aligned", what);
    return ENERF_OK;
}

struct CompositeRun {
    const enerf_composite_frame_args_t* a = nullptr;
    const enerf_composite_cache_t* cache = nullptr;  // cached frame: the maps, texels and cameras come from here
    const int* view_idx = nullptr;
    bool moving = false;                 // the boxes' positions are bbox_xy on the device (enerf_forward_composite_moving)
    const float* bbox_xy = nullptr;
    int* flags_out = nullptr;
    CompositePlan P;
    hipStream_t st = nullptr;            // the caller's stream
    float* ws = nullptr;
    int L = 0;
    SideLane* lane = nullptr;
    std::unique_lock<std::mutex> lane_busy;          // held until this call has enqueued its last join (side_lane.h)
    bool forked = false;
    bool dirty[kLaneStreams] = {false, false, false};     // the lane stream has launches the caller's stream has not waited for
    // hand-off from level i - 1 to level i, per cascade
    const float *pdepth[kCompCascades] = {}, *pstd[kCompCascades] = {}, *pnf[kCompCascades] = {};
    int hp = 0, wp = 0;

    const enerf_cascade_t& cas() const { return a->cas; }
    LaneStream lane_of(int k) const { return !forked || k == L ? kLaneMain : (k & 1) ? kLaneRender : kLaneSide; }
    LaneStream lane_of_sources() const { return forked ? kLaneSide : kLaneMain; }
    hipStream_t on(LaneStream s) {       // the stream to enqueue on; a lane stream is un-joined from here on
        if (s == kLaneMain) return st;
        dirty[s] = true;
        return lane->stream[s];
    }
    void join() {                        // the caller's stream waits for everything enqueued on the lane so far
        if (dirty[kLaneSide]) { lane->record(kEvSideDone, kLaneSide); lane->wait(kLaneMain, kEvSideDone); dirty[kLaneSide] = false; }
        if (dirty[kLaneRender]) { lane->record(kEvDone, kLaneRender); lane->wait(kLaneMain, kEvDone); dirty[kLaneRender] = false; }
    }
    // Error exit.  The plan repeats every refusal of the stage entries that depends on the arguments alone (shapes, windows, sample
    // counts, the raw render's limits), so none of those is left for behind the fork, and the tests find none; what can still fail
    // there is a launch error or a layer shape no convolution kernel takes.  Such an exit leaves through here: the caller's stream
    // never returns ahead of a lane stream, whether or not that stream got a launch yet (FrameRun::bail's pattern).
    int bail(int code) { join(); return code; }
    int finish() { join(); return check_launch("forward_composite"); }
    float* depth_of(int i, int k) const { return a->depth_map[i][k] ? a->depth_map[i][k] : ws + P.C[i][k].depth; }
    float* std_of(int i, int k) const { return a->std_map[i][k] ? a->std_map[i][k] : ws + P.C[i][k].std; }
    const float* rays_of(int i) const { return a->rays[i] ? a->rays[i] : ws + P.L[i].rays; }
    // the source cameras of the raw renders: the batch's, or (cached frame) the rows the preparation leaves in the workspace
    const float* src_exts() const { return cache ? ws + P.cam_exts : a->src_exts; }
    const float* src_ixts() const { return cache ? ws + P.cam_ixts : a->src_ixts; }
    // moving boxes: where the preparation leaves layer l's corner at level i (render = 0: volume grid, 1: ray raster); else nullptr
    const int* corner_of(int i, int render, int l) const {
        return moving ? reinterpret_cast<const int*>(ws + P.wintab) + win_table_at(i, render, l) : nullptr;
    }

    // the plan, and everything the host can refuse before the first launch
    int begin(const enerf_composite_frame_args_t* args, const enerf_composite_cache_t* k, const int* idx, enerf_stream_t stream) {
        a = args; cache = k; view_idx = idx;
        if (int rc = make_composite_plan(a, &P, cache != nullptr, moving)) return rc;
        if (moving) REQUIRE(bbox_xy, "forward_composite_moving: null bbox_xy (an (L,2) float32 device array: x, y of every layer's box)");
        if (cache != nullptr) {
            if (int rc = check_composite_cache("forward_composite_cached", cache, a->cas, a->H, a->W)) return rc;
            REQUIRE(view_idx, "forward_composite_cached: null view_idx (an (S) int32 device array)");
        }
        REQUIRE(a->workspace, "forward_composite: workspace is null");
        REQUIRE((uintptr_t)a->workspace % 16 == 0, "forward_composite: workspace must be 16-byte aligned");
        if (a->workspace_bytes < P.total_floats * sizeof(float))
            return fail(ENERF_EWORKSPACE, "forward_composite: workspace too small (%zu < %zu bytes)", a->workspace_bytes,
                        P.total_floats * sizeof(float));
        st = (hipStream_t)stream;
        ws = (float*)a->workspace;
        L = a->L;
        return ENERF_OK;
    }

    // ---- everything that depends on the cameras, near_far and the boxes alone, on the caller's stream in front of the fork: the
    // preparation launch (all proj, level 0's planes of every cascade, every window's ray list) and the generated rays.  A cached
    // frame's launch reads the source cameras from the cache's tables through view_idx and writes the gathered rows beside the rest
    int prep() {
        const enerf_cascade_t& c = cas();
        enerf_composite_prep_t p;
        memset(&p, 0, sizeof(p));
        p.src_ixts = cache ? cache->ixts : a->src_ixts; p.src_exts = cache ? cache->exts : a->src_exts;
        p.tar_ixt = a->tar_ixt; p.tar_ext = a->tar_ext; p.near_far = a->near_far;
        p.L = L; p.S = a->S; p.num_levels = c.num;
        p.fg_planes = P.C[0][0].D; p.bg_planes = P.C[0][L].D; p.h = P.L[0].h; p.w = P.L[0].w; p.depth_inv = c.depth_inv[0];
        for (int k = 0; k <= L; ++k) { p.dv[k] = ws + P.C[0][k].dv; p.nf[k] = ws + P.C[0][k].nf; }
        for (int i = 0; i < c.num; ++i) {
            const CompLevel& V = P.L[i];
            p.src_scale[i] = (float)c.im_feat_scale[i]; p.tar_scale[i] = (float)c.volume_scale[i]; p.proj[i] = ws + V.proj;
            if (!V.render) continue;
            p.Hr[i] = V.Hr; p.Wr[i] = V.Wr;
            for (int l = 0; l < L; ++l) {
                for (int q = 0; q < 4; ++q) p.win[i][l][q] = V.rwin[l][q];
                p.index[i][l] = (int*)(ws + P.C[i][l].index); p.count[i][l] = (int*)(ws + P.C[i][l].count);
            }
        }
        CompositePrep job;
        if (int rc = composite_prep_job(&p, &job)) return rc;
        if (cache != nullptr) {
            job.view_idx = view_idx; job.V = cache->V; job.cam_exts = ws + P.cam_exts; job.cam_ixts = ws + P.cam_ixts;
            job.invalid = (int*)(ws + P.invalid);
        }
        if (moving) {                                // (job.win[j].level / .layer name the window; its x0, y0 are 0 and unread)
            MovingBoxes& M = job.mv;
            M.xy = bbox_xy; M.table = (int*)(ws + P.wintab); M.flags = M.table + kWinTableInts; M.flags_out = flags_out;
            M.L = L; M.num_levels = c.num; M.H = a->H; M.W = a->W;
            for (int l = 0; l < L; ++l) { M.bw[l] = P.bw[l]; M.bh[l] = P.bh[l]; }
            for (int i = 0; i < c.num; ++i) {
                const CompLevel& V = P.L[i];
                M.vscale[i] = (float)c.volume_scale[i]; M.rscale[i] = (float)c.render_scale[i];
                for (int l = 0; l < L; ++l) {
                    M.vroom[i][l][0] = V.w - V.vwin[l][2]; M.vroom[i][l][1] = V.h - V.vwin[l][3];
                    M.rroom[i][l][0] = V.render ? V.Wr - V.rwin[l][2] : -1; M.rroom[i][l][1] = V.render ? V.Hr - V.rwin[l][3] : -1;
                }
            }
        }
        launch_composite_prep(job, st);
        if (int rc = check_launch("forward_composite: prep")) return rc;
        for (int i = 0; i < c.num; ++i) {
            const CompLevel& V = P.L[i];
            if (!V.render || a->rays[i] != nullptr) continue;
            if (int rc = enerf_gen_rays(a->tar_ext, a->tar_ixt, 1, V.Hr, V.Wr, (float)c.render_scale[i], ws + V.rays, st)) return rc;
        }
        return ENERF_OK;
    }

    // ---- the fork: the lane streams start behind the preparation (and with it behind whatever the caller's stream held before)
    void fork() {
        if (a->options && a->options->single_stream) return;
        lane = side_lane(st);
        if (lane == nullptr) return;
        lane_busy = std::unique_lock<std::mutex>(lane->busy);
        lane->record(kEvFork, kLaneMain);
        lane->wait(kLaneSide, kEvFork);
        dirty[kLaneSide] = true;                     // forked = to be joined, launches or not: an error exit in front of a stream's first
        if (L >= 2) { lane->wait(kLaneRender, kEvFork); dirty[kLaneRender] = true; }      // launch must not leave it un-joined (stream capture)
        forked = true;
    }

    // ---- sources: the two FeatureNets (feature_net.py:27-36, level_2 as plain features; both over src_inps) and every rendered level's
    // texel images (the background's take their colours from bg_src_inps);
    // the foreground's on the side stream, `feats` telling the render stream's layers they are there
    int sources_of(const float* packed, const float* rgb, const size_t* f, size_t featws, bool fg, LaneStream s) {
        const FeatDims fd(a->H, a->W);
        const float* img = a->src_inps;              // BOTH nets read src_inps (network_composite.py:78-79); bg_src_inps only colours
        if (int rc = feature_net_stage_job(packed, img, a->S, a->H, a->W, ws + f[0], ws + f[1], ws + f[2], 8, ws + featws, P.featws_bytes,
                                           ENERF_FEAT_ALL, a->options, on(s), nullptr, nullptr))
            return rc;
        for (int i = 0; i < cas().num; ++i) {
            const CompLevel& V = P.L[i];
            if (!V.render) continue;
            if (int rc = enerf_pack_texels_cl(ws + f[V.fl], fd.c[V.fl], rgb, a->H, a->W, V.Hr, V.Wr, tex_stride(V.F), a->S,
                                              ws + (fg ? V.tex_fg : V.tex_bg), on(s)))
                return rc;
        }
        return ENERF_OK;
    }
    // cached frame: one net's sources = one gather launch of the selected views' maps (the levels a cost volume reads) and texel images
    // (the cameras came with the preparation)
    int gather_of(float* const* feat, float* const* tex, const size_t* f, bool fg, LaneStream s) {
        const FeatDims fd(a->H, a->W);
        GatherJob J;
        memset(&J, 0, sizeof(J));
        J.V = cache->V; J.view_idx = view_idx;
        auto add = [&J](const float* src, float* dst, long long floats_per_view) {
            J.seg[J.nseg++] = GatherSeg{reinterpret_cast<const float4*>(src), reinterpret_cast<float4*>(dst), floats_per_view / 4};
        };
        for (int i = 0; i < cas().num; ++i) add(feat[i], ws + f[i], fd.pixels(i) * fd.c[i]);
        for (int i = 0; i < cas().num; ++i) {
            const CompLevel& V = P.L[i];
            if (V.render) add(tex[i], ws + (fg ? V.tex_fg : V.tex_bg), (long long)V.Hr * V.Wr * tex_stride(V.F));
        }
        launch_gather_sources(J, a->S, on(s));
        return check_launch("forward_composite_cached: gather");
    }
    int sources() {
        int rc = cache ? gather_of(cache->fg_feat, cache->fg_tex, P.f_fg, true, lane_of_sources())
                       : sources_of(a->feature_net_packed, a->src_inps, P.f_fg, P.featws_fg, true, lane_of_sources());
        if (forked && L >= 2) { lane->record(kEvFeats, kLaneSide); lane->wait(kLaneRender, kEvFeats); }
        if (rc != ENERF_OK) return rc;
        return cache ? gather_of(cache->bg_feat, cache->bg_tex, P.f_bg, false, kLaneMain)
                     : sources_of(a->feature_net_bg_packed, a->bg_src_inps, P.f_bg, P.featws_bg, false, kLaneMain);
    }

    // ---- cascade k, level i, up to its depth / std maps (network_composite.py:83-113): depth planes (level 0's came with the
    // preparation), the cost volume — of the layer's window only —, MinCostRegNet, the regression over the whole grid
    int cascade_level(int i, int k) {
        const CompLevel& V = P.L[i];
        const CompCascadeLevel& K = P.C[i][k];
        const bool fg = k < L;
        hipStream_t s = on(lane_of(k));
        float *dv = ws + K.dv, *nf = ws + K.nf, *vol = ws + K.vol, *prob = ws + K.prob, *depth = depth_of(i, k), *std = std_of(i, k);
        const float* feat = ws + (fg ? P.f_fg : P.f_bg)[i];
        const float* proj = ws + V.proj;
        int rc = ENERF_OK;
        if (i > 0)
            rc = enerf_get_depth_values(a->near_far + 2 * k, pdepth[k], pstd[k], pnf[k], 1, K.D, V.h, V.w, hp, wp, V.inv, dv, nf, s);
        if (rc != ENERF_OK) return rc;
        const int* wn = V.vwin[k];
        const int* at = fg ? corner_of(i, 0, k) : nullptr;         // moving boxes: the corner is read on the device
        rc = !fg  ? enerf_build_feature_volume(feat, proj, dv, 1, a->S, V.C, V.Hs, V.Ws, K.D, V.h, V.w, vol, s)
             : at ? enerf_build_feature_volume_window_at(feat, proj, dv, 1, a->S, V.C, V.Hs, V.Ws, K.D, V.h, V.w, at, wn[2], wn[3], vol, s)
                  : enerf_build_feature_volume_window(feat, proj, dv, 1, a->S, V.C, V.Hs, V.Ws, K.D, V.h, V.w, wn[0], wn[1], wn[2], wn[3], vol, s);
        if (rc != ENERF_OK) return rc;
        rc = cost_reg_run(a->cost_reg_packed[i][k], V.C, 0, vol, 0, 1, K.D, K.wh, K.ww, ws + K.feat3d, prob, ws + P.costreg_ws[k],
                          P.costreg_ws_bytes[k], a->options, s);              // (feat3d: dead work)
        if (rc != ENERF_OK) return rc;
        rc = !fg  ? enerf_depth_regression(prob, dv, 1, K.D, V.h, V.w, V.inv, depth, std, s)
             : at ? enerf_depth_regression_window_at(prob, dv, 1, K.D, V.h, V.w, at, wn[2], wn[3], V.inv, depth, std, s)
                  : enerf_depth_regression_window(prob, dv, 1, K.D, V.h, V.w, wn[0], wn[1], wn[2], wn[3], V.inv, depth, std, s);
        pdepth[k] = depth; pstd[k] = std; pnf[k] = nf;
        return rc;
    }

    // ---- cascade k, rendered level i: the raw samples of the layer's window (the background: of the whole raster) ----
    int raw_render(int i, int k) {
        const CompLevel& V = P.L[i];
        const CompCascadeLevel& K = P.C[i][k];
        const bool fg = k < L;
        enerf_render_raw_args_t r;
        memset(&r, 0, sizeof(r));
        r.rays8 = rays_of(i); r.depth_map = pdepth[k]; r.std_map = pstd[k]; r.nf_map = pnf[k]; r.map_h = V.h; r.map_w = V.w;
        r.tex = ws + (fg ? V.tex_fg : V.tex_bg); r.vol = nullptr;
        r.src_exts = src_exts(); r.src_ixts = src_ixts(); r.tar_ext = a->tar_ext; r.packed = a->nerf_packed[i][k];
        r.raw = ws + K.raw; r.z = ws + K.z;
        r.B = 1; r.N = V.Hr * V.Wr; r.S = a->S; r.n_samples = V.Ns; r.depth_inv = V.inv; r.Hr = V.Hr; r.Wr = V.Wr; r.F = V.F;
        r.render_scale = (float)cas().render_scale[i];
        if (fg) { r.ray_index = (const int*)(ws + K.index); r.ray_count = (const int*)(ws + K.count); }
        return enerf_render_rays_raw(&r, on(lane_of(k)));
    }

    // ---- rendered level i: parse_layer + raw2outputs_composite over the L layers' and the background's samples, behind the join ----
    int merge(int i) {
        const CompLevel& V = P.L[i];
        join();
        enerf_composite_layers_t m;
        memset(&m, 0, sizeof(m));
        for (int l = 0; l < L; ++l) {
            m.fg_raw[l] = ws + P.C[i][l].raw; m.fg_z[l] = ws + P.C[i][l].z;
            for (int q = 0; q < 4; ++q) m.win[l][q] = V.rwin[l][q];
        }
        m.bg_raw = ws + P.C[i][L].raw; m.bg_z = ws + P.C[i][L].z;
        m.L = L; m.Ns = V.Ns; m.H = V.Hr; m.W = V.Wr; m.white_bkgd = 0;
        m.rgb = a->rgb[i]; m.depth = a->depth[i]; m.weights = a->weights[i]; m.net_output = a->net_output[i]; m.z_vals = a->z_vals[i];
        // (uncached, boxes on the host: enerf_composite_layers itself; moving boxes: the L corners of this level's raster, on the device)
        return composite_layers_run_at(&m, cache ? (const int*)(ws + P.invalid) : nullptr, corner_of(i, 1, 0), st);
    }
};

int run_composite(const enerf_composite_frame_args_t* a, const enerf_composite_cache_t* cache, const int* view_idx, enerf_stream_t stream,
                  bool moving = false, const float* bbox_xy = nullptr, int* flags = nullptr) {
    CompositeRun R;
    R.moving = moving; R.bbox_xy = bbox_xy; R.flags_out = flags;
    int rc = R.begin(a, cache, view_idx, stream);
    if (rc != ENERF_OK) return rc;
    rc = R.prep();
    if (rc != ENERF_OK) return rc;                 // (nothing forked yet)
    R.fork();
    rc = R.sources();
    if (rc != ENERF_OK) return R.bail(rc);
    for (int i = 0; i < a->cas.num; ++i) {
        const bool render = R.P.L[i].render != 0;
        for (int k = 0; k <= a->L && rc == ENERF_OK; ++k) {       // the layers first: their lane streams get their work early
            rc = R.cascade_level(i, k);
            if (rc == ENERF_OK && render) rc = R.raw_render(i, k);
        }
        if (rc == ENERF_OK && render) rc = R.merge(i);
        if (rc != ENERF_OK) return R.bail(rc);
        R.hp = R.P.L[i].h; R.wp = R.P.L[i].w;
    }
    return R.finish();
}
}  // namespace
}  // namespace enerf

extern "C" {

size_t enerf_mask_compact_workspace_bytes(long long n) { return mask_compact_workspace_bytes(n); }
int enerf_mask_compact(const void* mask, int elem_bytes, long long n, int* index, int* count, void* workspace,
                       size_t workspace_bytes, enerf_stream_t stream) {
    REQUIRE(mask && index && count && workspace && n > 0, "mask_compact: bad arguments");
    REQUIRE(n < (1LL << 31), "mask_compact: more than 2^31 elements");
    REQUIRE(elem_bytes == 1 || elem_bytes == 2 || elem_bytes == 4 || elem_bytes == 8, "mask_compact: elem_bytes=%d unsupported", elem_bytes);
    if (workspace_bytes < mask_compact_workspace_bytes(n)) return fail(ENERF_EWORKSPACE, "mask_compact: workspace too small");
    launch_mask_compact(mask, elem_bytes, n, index, count, workspace, (hipStream_t)stream);
    return check_launch("mask_compact");
}

size_t enerf_forward_workspace_bytes(const enerf_frame_args_t* a) {
    FramePlan P;
    if (make_plan(a, &P) != ENERF_OK) return 0;
    return P.total_floats * sizeof(float);
}

int enerf_forward(const enerf_frame_args_t* a, enerf_stream_t stream) { return run_frame(a, nullptr, nullptr, stream); }

size_t enerf_forward_cached_workspace_bytes(const enerf_frame_args_t* a, const enerf_source_cache_t* cache) {
    FramePlan P;
    if (make_plan(a, &P, true) != ENERF_OK) return 0;
    if (check_cache("forward_cached", cache, a->cas, a->H, a->W) != ENERF_OK) return 0;
    return P.total_floats * sizeof(float);
}

int enerf_forward_cached(const enerf_frame_args_t* a, const enerf_source_cache_t* cache, const int* view_idx, enerf_stream_t stream) {
    REQUIRE(cache, "forward_cached: null cache");
    return run_frame(a, cache, view_idx, stream);
}

// ---- the cache itself: sizes for a cascade, and the build (FeatureNet + texel packing over the V views, <= 4 at a time) ----
int enerf_source_cache_sizes(const enerf_cascade_t* cas, int V, int H, int W, int* l2_stride_out, long long* floats) {
    REQUIRE(cas && l2_stride_out && floats, "source_cache_sizes: null pointer");
    const enerf_cascade_t& c = *cas;
    REQUIRE(c.num >= 1 && c.num <= ENERF_MAX_LEVELS, "source_cache_sizes: cas_config.num=%d unsupported (1..%d)", c.num, ENERF_MAX_LEVELS);
    REQUIRE(V >= 1 && H > 0 && W > 0 && H % 4 == 0 && W % 4 == 0, "source_cache_sizes: bad shape V=%d H=%d W=%d (H and W divisible by 4)", V, H, W);
    const int tex2 = cascade_tex2(c);
    const FeatDims fd(H, W);
    *l2_stride_out = l2_stride(tex2);
    for (int l = 0; l < 3; ++l) floats[l] = (long long)V * fd.pixels(l) * (l == 2 ? l2_stride(tex2) : fd.c[l]);
    for (int i = 0; i < ENERF_MAX_LEVELS; ++i) {
        floats[3 + i] = 0;
        if (i >= c.num || !c.render_if[i]) continue;
        const int Hr = scaled(H, c.render_scale[i]), Wr = scaled(W, c.render_scale[i]);
        const int rc = check_render_feat("source_cache_sizes", c, i, fd, Hr, Wr, true);
        if (rc != ENERF_OK) return rc;
        if (renders_from_l2(c, i, tex2)) continue;
        floats[3 + i] = (long long)V * Hr * Wr * tex_stride(c.nerf_model_feat_ch[i] + 3);
    }
    floats[6] = (long long)V * 16;
    floats[7] = (long long)V * 9;
    return ENERF_OK;
}

size_t enerf_source_cache_build_workspace_bytes(int H, int W) { return enerf_feature_net_workspace_bytes(4, H, W); }

int enerf_source_cache_build(const enerf_source_cache_t* cache, const float* src_inps, const float* exts, const float* ixts,
                             const float* feature_net_packed, const enerf_cascade_t* cas, int chunk, void* workspace,
                             size_t workspace_bytes, const enerf_options_t* options, enerf_stream_t stream) {
    REQUIRE(cache && cas, "source_cache_build: null cache / cascade");
    REQUIRE(src_inps && exts && ixts && feature_net_packed && workspace, "source_cache_build: null pointer");
    if (chunk == 0) chunk = 4;
    REQUIRE(chunk >= 1 && chunk <= 4, "source_cache_build: chunk=%d (1..4 images per FeatureNet call)", chunk);
    const int V = cache->V, H = cache->H, W = cache->W;
    long long floats[ENERF_SOURCE_CACHE_BUFFERS];
    int l2s = 0;
    int rc = enerf_source_cache_sizes(cas, V, H, W, &l2s, floats);
    if (rc != ENERF_OK) return rc;
    rc = check_cache("source_cache_build", cache, *cas, H, W);
    if (rc != ENERF_OK) return rc;
    if (workspace_bytes < enerf_source_cache_build_workspace_bytes(H, W))
        return fail(ENERF_EWORKSPACE, "source_cache_build: workspace too small");
    const FeatDims fd(H, W);
    float* maps[3] = {cache->feat_l0, cache->feat_l1, cache->feat_l2};
    for (int v0 = 0; v0 < V; v0 += chunk) {
        const int n = V - v0 < chunk ? V - v0 : chunk;
        const float* img = src_inps + (size_t)v0 * 3 * H * W;
        float* m[3];
        for (int l = 0; l < 3; ++l) m[l] = maps[l] + (size_t)v0 * fd.pixels(l) * (l == 2 ? l2s : fd.c[l]);
        rc = enerf_feature_net(feature_net_packed, img, n, H, W, m[0], m[1], m[2], l2s, workspace, workspace_bytes, options, stream);
        if (rc != ENERF_OK) return rc;
        for (int i = 0; i < cas->num; ++i) {
            if (floats[3 + i] == 0) continue;
            const int fl = cas->render_im_feat_level[i], TEX = tex_stride(fd.c[fl] + 3);
            rc = enerf_pack_texels_cl(m[fl], fd.c[fl], img, H, W, fd.h[fl], fd.w[fl], TEX, n, cache->tex[i] + (size_t)v0 * fd.pixels(fl) * TEX, stream);
            if (rc != ENERF_OK) return rc;
        }
    }
    GatherJob J;                                        // the cameras: slot v takes view v
    memset(&J, 0, sizeof(J));
    J.V = V; J.exts = exts; J.ixts = ixts; J.dst_exts = cache->exts; J.dst_ixts = cache->ixts;
    launch_gather_sources(J, V, (hipStream_t)stream);
    return check_launch("source_cache_build");
}

// ---- the composite network in one call ----
size_t enerf_forward_composite_workspace_bytes(const enerf_composite_frame_args_t* a) {
    CompositePlan P;
    if (make_composite_plan(a, &P) != ENERF_OK) return 0;
    return P.total_floats * sizeof(float);
}

int enerf_forward_composite(const enerf_composite_frame_args_t* a, enerf_stream_t stream) { return run_composite(a, nullptr, nullptr, stream); }

size_t enerf_forward_composite_cached_workspace_bytes(const enerf_composite_frame_args_t* a, const enerf_composite_cache_t* cache) {
    CompositePlan P;
    if (make_composite_plan(a, &P, true) != ENERF_OK) return 0;
    if (check_composite_cache("forward_composite_cached", cache, a->cas, a->H, a->W) != ENERF_OK) return 0;
    return P.total_floats * sizeof(float);
}

int enerf_forward_composite_cached(const enerf_composite_frame_args_t* a, const enerf_composite_cache_t* cache, const int* view_idx,
                                   enerf_stream_t stream) {
    REQUIRE(cache, "forward_composite_cached: null cache");
    return run_composite(a, cache, view_idx, stream);
}

// ---- the composite frame with boxes that move: bbox[l][2..3] of the argument block are the sizes (bbox[l][0..1] are ignored), the
// positions are bbox_xy (L,2) float32 on the device, read by the kernels; flags (L) int32 on the device, optional
size_t enerf_forward_composite_moving_workspace_bytes(const enerf_composite_frame_args_t* a) {
    CompositePlan P;
    if (make_composite_plan(a, &P, false, true) != ENERF_OK) return 0;
    return P.total_floats * sizeof(float);
}
int enerf_forward_composite_moving(const enerf_composite_frame_args_t* a, const float* bbox_xy, int* flags, enerf_stream_t stream) {
    return run_composite(a, nullptr, nullptr, stream, true, bbox_xy, flags);
}
size_t enerf_forward_composite_cached_moving_workspace_bytes(const enerf_composite_frame_args_t* a, const enerf_composite_cache_t* cache) {
    CompositePlan P;
    if (make_composite_plan(a, &P, true, true) != ENERF_OK) return 0;
    if (check_composite_cache("forward_composite_cached", cache, a->cas, a->H, a->W) != ENERF_OK) return 0;
    return P.total_floats * sizeof(float);
}
int enerf_forward_composite_cached_moving(const enerf_composite_frame_args_t* a, const enerf_composite_cache_t* cache, const int* view_idx,
                                          const float* bbox_xy, int* flags, enerf_stream_t stream) {
    REQUIRE(cache, "forward_composite_cached: null cache");
    return run_composite(a, cache, view_idx, stream, true, bbox_xy, flags);
}

// ---- the composite cache itself: sizes for a cascade, and the build (per net the frame's FeatureNet and texel-pack calls over the V
// views, <= 4 at a time; a map the cache does not keep lives in the workspace for the length of its chunk) ----
int enerf_composite_cache_sizes(const enerf_cascade_t* cas, int V, int H, int W, long long* floats) {
    REQUIRE(cas && floats, "composite_cache_sizes: null pointer");
    const enerf_cascade_t& c = *cas;
    REQUIRE(c.num >= 1 && c.num <= ENERF_MAX_LEVELS, "composite_cache_sizes: cas.num=%d unsupported (1..%d)", c.num, ENERF_MAX_LEVELS);
    REQUIRE(V >= 1 && H > 0 && W > 0 && H % 4 == 0 && W % 4 == 0, "composite_cache_sizes: bad shape V=%d H=%d W=%d (H and W divisible by 4)", V, H, W);
    const FeatDims fd(H, W);
    for (int i = 0; i < ENERF_COMPOSITE_CACHE_BUFFERS; ++i) floats[i] = 0;
    for (int i = 0; i < c.num; ++i) {
        floats[i] = floats[6 + i] = (long long)V * fd.pixels(i) * fd.c[i];
        if (!c.render_if[i]) continue;
        const int Hr = scaled(H, c.render_scale[i]), Wr = scaled(W, c.render_scale[i]);
        if (int rc = check_render_feat("composite_cache_sizes", c, i, fd, Hr, Wr, true)) return rc;
        floats[3 + i] = floats[9 + i] = (long long)V * Hr * Wr * tex_stride(c.nerf_model_feat_ch[i] + 3);
    }
    floats[12] = (long long)V * 16;
    floats[13] = (long long)V * 9;
    return ENERF_OK;
}

// the FeatureNet workspace of 4 images, then the three maps of 4 images (a net writes all three; the cache keeps some)
static size_t composite_cache_scratch_map(int H, int W, int l) {
    const FeatDims fd(H, W);
    size_t off = enerf_feature_net_workspace_bytes(4, H, W) / sizeof(float);
    for (int k = 0; k < l; ++k) off += (size_t)4 * fd.pixels(k) * fd.c[k];
    return off;
}
size_t enerf_composite_cache_build_workspace_bytes(int H, int W) { return composite_cache_scratch_map(H, W, 3) * sizeof(float); }

int enerf_composite_cache_build(const enerf_composite_cache_t* cache, const float* src_inps, const float* bg_src_inps, const float* exts,
                                const float* ixts, const float* feature_net_packed, const float* feature_net_bg_packed,
                                const enerf_cascade_t* cas, int chunk, void* workspace, size_t workspace_bytes,
                                const enerf_options_t* options, enerf_stream_t stream) {
    REQUIRE(cache && cas, "composite_cache_build: null cache / cascade");
    REQUIRE(src_inps && bg_src_inps && exts && ixts && feature_net_packed && feature_net_bg_packed && workspace,
            "composite_cache_build: null pointer");
    if (chunk == 0) chunk = 4;
    REQUIRE(chunk >= 1 && chunk <= 4, "composite_cache_build: chunk=%d (1..4 images per FeatureNet call)", chunk);
    const int V = cache->V, H = cache->H, W = cache->W;
    long long floats[ENERF_COMPOSITE_CACHE_BUFFERS];
    if (int rc = enerf_composite_cache_sizes(cas, V, H, W, floats)) return rc;
    if (int rc = check_composite_cache("composite_cache_build", cache, *cas, H, W)) return rc;
    REQUIRE((uintptr_t)workspace % 16 == 0, "composite_cache_build: workspace must be 16-byte aligned");
    if (workspace_bytes < enerf_composite_cache_build_workspace_bytes(H, W))
        return fail(ENERF_EWORKSPACE, "composite_cache_build: workspace too small");
    const FeatDims fd(H, W);
    const size_t featws_bytes = enerf_feature_net_workspace_bytes(4, H, W);
    for (int v0 = 0; v0 < V; v0 += chunk) {
        const int n = V - v0 < chunk ? V - v0 : chunk;
        const float* img = src_inps + (size_t)v0 * 3 * H * W;          // BOTH nets read src_inps; bg_src_inps only colours
        for (int net = 0; net < 2; ++net) {
            float* const* feat = net == 0 ? cache->fg_feat : cache->bg_feat;
            float* const* tex = net == 0 ? cache->fg_tex : cache->bg_tex;
            const float* rgb = (net == 0 ? src_inps : bg_src_inps) + (size_t)v0 * 3 * H * W;
            float* m[3];
            for (int l = 0; l < 3; ++l)
                m[l] = l < cas->num ? feat[l] + (size_t)v0 * fd.pixels(l) * fd.c[l] : (float*)workspace + composite_cache_scratch_map(H, W, l);
            if (int rc = feature_net_stage_job(net == 0 ? feature_net_packed : feature_net_bg_packed, img, n, H, W, m[0], m[1], m[2], 8, workspace,
                                               featws_bytes, ENERF_FEAT_ALL, options, (hipStream_t)stream, nullptr, nullptr))
                return rc;
            for (int i = 0; i < cas->num; ++i) {
                if (!cas->render_if[i]) continue;
                const int fl = cas->render_im_feat_level[i], TEX = tex_stride(fd.c[fl] + 3);
                if (int rc = enerf_pack_texels_cl(m[fl], fd.c[fl], rgb, H, W, fd.h[fl], fd.w[fl], TEX, n,
                                                  tex[i] + (size_t)v0 * fd.pixels(fl) * TEX, stream))
                    return rc;
            }
        }
    }
    GatherJob J;                                        // the cameras: slot v takes view v
    memset(&J, 0, sizeof(J));
    J.V = V; J.exts = exts; J.ixts = ixts; J.dst_exts = cache->exts; J.dst_ixts = cache->ixts;
    launch_gather_sources(J, V, (hipStream_t)stream);
    return check_launch("composite_cache_build");
}

}  // extern "C"
