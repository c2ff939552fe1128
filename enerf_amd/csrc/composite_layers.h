// composite_layers.h — the device code only the composite network (network_composite.py) needs; included by geometry.hip,
// which holds the softmax moments the windowed regression shares with k_depth_regression.
//   * k_depth_regression_window  depth_regression (utils.py:658-667) of a prob that exists only inside a layer's box
//                                (network_composite.py:100-102: F.pad then depth_regression), without the padded prob
//   * k_window_ray_index         the ray positions of a box in the render image (build_rays_composite), as the index list the
//                                render kernel's device-side selection reads
//   * k_composite_layers         parse_layer + raw2outputs_composite (utils.py:875-942): scatter, per-ray depth sort of the
//                                foreground samples, background appended, alpha compositing — one thread per pixel
//   * k_composite_layers_bwd     its backward (the training step): the gradients of every layer's and the background's raw samples
//   * k_depth_regression_window_at, k_composite_layers_at   the two forward kernels with their windows' corners read from device
//                                memory (boxes that move: prep_job.h resolves the positions, enerf_forward_composite_moving)
// (The windowed cost volume is k_feature_volume_mp<CQ, true> in volume.hip, the raw-sample render k_render_rays<..., RAW> in
// render.hip, the backwards of the windowed volume and regression k_feature_volume_bwd<CQ, true> and k_depth_regression_bwd<MK, true>
// in backward.hip: each is a template value of the kernel it shares its arithmetic with.)
#pragma once
#include <math.h>

namespace enerf {

// prob (B, D, wh, ww) of the window at (x0, y0); dv (B, D, h, w); depth / std (B, h, w).  k_depth_regression's mapping (a wave =
// 16 pixels x 4 depth slices) over the FULL grid; a pixel outside the window runs the same moments with zero logits.
// (depth_regression_window_body is inlined into both kernels: the scalar-argument one compiles to the code it was before the split.)
__device__ __forceinline__ void depth_regression_window_body(const float* __restrict__ prob, const float* __restrict__ dv, int B,
                                                             int D, int h, int w, int x0, int y0, int ww, int wh, int depth_inv,
                                                             float* __restrict__ depth, float* __restrict__ std) {
    const int lane = threadIdx.x & 63, sl = lane >> 4;
    const long long wave = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int hw = h * w, hwp = wh * ww;
    const long long i = wave * 16 + (lane & 15);
    const bool ok = i < (long long)B * hw;
    const long long ii = ok ? i : 0;
    const int b = (int)(ii / hw), p = (int)(ii - (long long)b * hw);
    const int y = p / w, x = p - y * w;
    const bool inside = x >= x0 && x < x0 + ww && y >= y0 && y < y0 + wh;
    const float* pr = prob + (long long)b * D * hwp + (inside ? (y - y0) * ww + (x - x0) : 0);
    const float* dp = dv + (long long)b * D * hw + p;
    float mu, var;
    if (D <= 16) depth_moments_regs<4>(pr, dp, D, hwp, hw, sl, depth_inv, !inside, mu, var);
    else depth_moments_regs<16>(pr, dp, D, hwp, hw, sl, depth_inv, !inside, mu, var);          // D <= 64 (the C-ABI layer checks)
    if (ok && sl == 0) {
        depth[i] = mu;
        std[i] = sqrtf(clamp_min(var, 1e-10f));
    }
}
__global__ __launch_bounds__(256) void k_depth_regression_window(const float* __restrict__ prob, const float* __restrict__ dv, int B,
                                                                 int D, int h, int w, int x0, int y0, int ww, int wh, int depth_inv,
                                                                 float* __restrict__ depth, float* __restrict__ std) {
    depth_regression_window_body(prob, dv, B, D, h, w, x0, y0, ww, wh, depth_inv, depth, std);
}
// the window's corner (x0, y0) = xy[0..1] on the device (moving boxes): one block-uniform load at kernel entry
__global__ __launch_bounds__(256) void k_depth_regression_window_at(const float* __restrict__ prob, const float* __restrict__ dv, int B,
                                                                    int D, int h, int w, const int* __restrict__ xy, int ww, int wh,
                                                                    int depth_inv, float* __restrict__ depth, float* __restrict__ std) {
    const int x0 = xy[0], y0 = xy[1];
    depth_regression_window_body(prob, dv, B, D, h, w, x0, y0, ww, wh, depth_inv, depth, std);
}
void launch_depth_regression_window_at(const float* prob, const float* dv, int B, int D, int h, int w, const int* xy, int ww, int wh,
                                       int depth_inv, float* depth, float* std, hipStream_t st) {
    const long long waves = cdivl((long long)B * h * w, 16);
    ENERF_LAUNCH(k_depth_regression_window_at, (unsigned)cdivl(waves, 4), 256, 0, st, prob, dv, B, D, h, w, xy, ww, wh, depth_inv, depth,
                 std);
}
void launch_depth_regression_window(const float* prob, const float* dv, int B, int D, int h, int w, int x0, int y0, int ww, int wh,
                                    int depth_inv, float* depth, float* std, hipStream_t st) {
    const long long waves = cdivl((long long)B * h * w, 16);
    ENERF_LAUNCH(k_depth_regression_window, (unsigned)cdivl(waves, 4), 256, 0, st, prob, dv, B, D, h, w, x0, y0, ww, wh, depth_inv, depth,
                 std);
}

// index[r] = the position in the (Hr, Wr) raster of the r-th pixel of the window, raster order; count[0] = ww * wh
__global__ __launch_bounds__(256) void k_window_ray_index(int x0, int y0, int ww, int wh, int Wr, int* __restrict__ index,
                                                          int* __restrict__ count) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0) count[0] = ww * wh;
    if (i >= ww * wh) return;
    const int yy = i / ww, xx = i - yy * ww;
    index[i] = (y0 + yy) * Wr + x0 + xx;
}
void launch_window_ray_index(int x0, int y0, int ww, int wh, int Wr, int* index, int* count, hipStream_t st) {
    ENERF_LAUNCH_SIMPLE(k_window_ray_index, (unsigned)cdiv(ww * wh, 256), 256, 0, st, x0, y0, ww, wh, Wr, index, count);
}

using CompositeLayers = enerf_composite_layers_t;
// Layer l's compact buffers hold the window's pixels in raster order; a pixel outside has zero samples (parse_layer).  With more
// than one layer the L * Ns foreground samples of the pixel are sorted by depth: an odd-even transposition network over NFP >=
// L * Ns register slots (padded with +inf, which stay last).  It exchanges NEIGHBOURS and only when the left one is strictly
// greater, so samples of equal depth keep their concatenation order (layer, then sample): the order is deterministic, where
// torch.sort promises none.  The background's Ns samples follow unsorted (utils.py:917-918).
// `invalid` (nullptr: none) is a device flag of the cached frame: nonzero = a source-view index was outside the cache, and every
// output of the level is NaN (the ReLUs upstream return 0 for NaN, so the views' NaN alone would reach the colours only).
// The body is composite_layers_body.h, shared as text with k_composite_layers_at below.
template <int NFP>
__global__ __launch_bounds__(256) void k_composite_layers(CompositeLayers a, const int* __restrict__ invalid) {
#define ENERF_CL_WIN_X(l) a.win[l][0]
#define ENERF_CL_WIN_Y(l) a.win[l][1]
#include "composite_layers_body.h"
#undef ENERF_CL_WIN_X
#undef ENERF_CL_WIN_Y
}
// Moving boxes (enerf_composite_layers_at): the corners of the L windows are on the device, (x0, y0) of layer l at
// win_xy[2 * l .. 2 * l + 1] — they replace a.win[l][0..1]; uniform loads at kernel entry and nothing else.
template <int NFP>
__global__ __launch_bounds__(256) void k_composite_layers_at(CompositeLayers a, const int* __restrict__ invalid,
                                                             const int* __restrict__ win_xy) {
#define ENERF_CL_WIN_X(l) (l < a.L ? win_xy[2 * l] : 0)
#define ENERF_CL_WIN_Y(l) (l < a.L ? win_xy[2 * l + 1] : 0)
#include "composite_layers_body.h"
#undef ENERF_CL_WIN_X
#undef ENERF_CL_WIN_Y
}
void launch_composite_layers_at(const CompositeLayers& a, hipStream_t st, const int* invalid, const int* win_xy) {
    const int nf = a.L * a.Ns;                          // launch_composite_layers' branch
    const unsigned grid = (unsigned)cdiv(a.H * a.W, 256);
    if (nf <= 2) ENERF_LAUNCH_SIMPLE(k_composite_layers_at<2>, grid, 256, 0, st, a, invalid, win_xy);
    else if (nf <= 4) ENERF_LAUNCH_SIMPLE(k_composite_layers_at<4>, grid, 256, 0, st, a, invalid, win_xy);
    else if (nf <= 8) ENERF_LAUNCH_SIMPLE(k_composite_layers_at<8>, grid, 256, 0, st, a, invalid, win_xy);
    else ENERF_LAUNCH_SIMPLE(k_composite_layers_at<16>, grid, 256, 0, st, a, invalid, win_xy);
}
void launch_composite_layers(const CompositeLayers& a, hipStream_t st, const int* invalid) {
    const int nf = a.L * a.Ns;
    const unsigned grid = (unsigned)cdiv(a.H * a.W, 256);
    if (nf <= 2) ENERF_LAUNCH_SIMPLE(k_composite_layers<2>, grid, 256, 0, st, a, invalid);
    else if (nf <= 4) ENERF_LAUNCH_SIMPLE(k_composite_layers<4>, grid, 256, 0, st, a, invalid);
    else if (nf <= 8) ENERF_LAUNCH_SIMPLE(k_composite_layers<8>, grid, 256, 0, st, a, invalid);
    else ENERF_LAUNCH_SIMPLE(k_composite_layers<16>, grid, 256, 0, st, a, invalid);      // L * Ns <= 16 (the C-ABI layer checks)
}

using CompositeLayersBwd = enerf_composite_layers_bwd_t;
// The backward of k_composite_layers, one thread per pixel: the pixel's stable depth order is recomputed exactly as the forward
// computes it (same network, same comparisons), then the T = (L + 1) * Ns samples are walked twice in composited order — forwards
// for the transmittance in front of every sample (Tk, the only per-sample state kept besides the order), backwards through
// the cumulative product as k_composite_bwd does (torch's cumprod backward; 1 - alpha + 1e-10 is never 0):
//   w_t = alpha_t Tk_t,  Tk_t = prod_{j<t} (1 - alpha_j + 1e-10),  alpha = 1 - exp(-sigma)
//   g w_t = g_weights[t] + g_depth z_t + g_rgb . c_t (- sum g_rgb with white_bkgd);   g c_t = w_t g_rgb
//   g alpha_t = g w_t Tk_t - (sum_{k>t} g w_k alpha_k Tk_k) / (1 - alpha_t + 1e-10);  g sigma_t = g alpha_t exp(-sigma_t)
// No gradient to any depth (the reference composites weights * z_vals.detach(), and a permutation has no derivative).  A layer's
// window row belongs to exactly one pixel and a pixel inside a layer's window meets each of the layer's Ns samples once in the
// sorted list: every row of every grad_fg_raw[l] and of grad_bg_raw is written once, by plain stores — the result does not depend on
// the launch.  Samples of a layer that does not cover the pixel are zeros (alpha 0): they take part in the walk and write nothing.
template <int NFP>
__global__ __launch_bounds__(256) void k_composite_layers_bwd(CompositeLayersBwd g) {
    const CompositeLayers& a = g.fwd;
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= a.H * a.W) return;
    const int y = p / a.W, x = p - y * a.W;
    const int Ns = a.Ns, nf = a.L * Ns, T = nf + Ns;   // Ns <= nf <= NFP: T <= 2 * NFP
    int base[ENERF_MAX_FG_LAYERS];
#pragma unroll
    for (int l = 0; l < ENERF_MAX_FG_LAYERS; ++l) {
        const int wx = a.win[l][0], wy = a.win[l][1], ww = a.win[l][2], wh = a.win[l][3];
        base[l] = (l < a.L && x >= wx && x < wx + ww && y >= wy && y < wy + wh) ? (y - wy) * ww + (x - wx) : -1;
    }
    auto row_of = [&](int l) { return l == 0 ? base[0] : (l == 1 ? base[1] : (l == 2 ? base[2] : base[3])); };
    auto z_of = [&](int l) { return l == 0 ? a.fg_z[0] : (l == 1 ? a.fg_z[1] : (l == 2 ? a.fg_z[2] : a.fg_z[3])); };
    auto raw_of = [&](int l) { return l == 0 ? a.fg_raw[0] : (l == 1 ? a.fg_raw[1] : (l == 2 ? a.fg_raw[2] : a.fg_raw[3])); };
    auto graw_of = [&](int l) {
        return l == 0 ? g.grad_fg_raw[0] : (l == 1 ? g.grad_fg_raw[1] : (l == 2 ? g.grad_fg_raw[2] : g.grad_fg_raw[3]));
    };
    float zk[NFP];
    int id[NFP];
#pragma unroll
    for (int i = 0; i < NFP; ++i) {
        zk[i] = INFINITY;
        id[i] = i;
        if (i < nf) {
            const int l = i / Ns, k = i - l * Ns, row = row_of(l);
            zk[i] = row >= 0 ? z_of(l)[(long long)row * Ns + k] : 0.f;
        }
    }
    if (a.L > 1) {                                      // uniform; the forward's network
#pragma unroll
        for (int r = 0; r < NFP; ++r)
#pragma unroll
            for (int i = r & 1; i + 1 < NFP; i += 2) {
                const bool sw = zk[i] > zk[i + 1];
                const float zl = zk[i], zr = zk[i + 1];
                const int il = id[i], ir = id[i + 1];
                zk[i] = sw ? zr : zl; zk[i + 1] = sw ? zl : zr;
                id[i] = sw ? ir : il; id[i + 1] = sw ? il : ir;
            }
    }
    // The walks below are runtime loops over T <= 2 * NFP samples (unrolled around register arrays they spill at NFP = 16): the
    // sorted order and the transmittances go through LDS columns only this thread touches ([.][threadIdx.x]: no barrier, no conflict).
    __shared__ unsigned char s_id[NFP][256];
    __shared__ float s_T[2 * NFP][256];
    const int tid = threadIdx.x;
#pragma unroll
    for (int i = 0; i < NFP; ++i) s_id[i][tid] = (unsigned char)id[i];
    // sample t of the composited order: where its [r, g, b, sigma] and its depth are read and its gradient is written (nullptr: a
    // zero sample of a layer that does not cover the pixel)
    auto locate = [&](int t, const float*& src, const float*& zsrc, float*& dst) {
        if (t >= nf) {
            const long long o = (long long)p * Ns + (t - nf);
            src = a.bg_raw + o * 4; zsrc = a.bg_z + o; dst = g.grad_bg_raw + o * 4;
            return;
        }
        const int sid = s_id[t][tid];
        const int l = sid / Ns, k = sid - l * Ns, row = row_of(l);
        src = nullptr; zsrc = nullptr; dst = nullptr;
        if (row >= 0) {
            const long long o = (long long)row * Ns + k;
            src = raw_of(l) + o * 4; zsrc = z_of(l) + o; dst = graw_of(l) + o * 4;
        }
    };
    float Tacc = 1.f;
    for (int t = 0; t < T; ++t) {
        const float *src, *zsrc; float* dst;
        locate(t, src, zsrc, dst);
        const float sigma = src != nullptr ? src[3] : 0.f;
        const float alpha = 1.f - expf(-sigma);
        s_T[t][tid] = Tacc;
        Tacc *= (1.f - alpha + 1e-10f);
    }
    const bool has_rgb = g.grad_rgb != nullptr;         // absent upstream gradients (nullptr) are zeros
    const float gr0 = has_rgb ? g.grad_rgb[(long long)p * 3 + 0] : 0.f, gr1 = has_rgb ? g.grad_rgb[(long long)p * 3 + 1] : 0.f;
    const float gr2 = has_rgb ? g.grad_rgb[(long long)p * 3 + 2] : 0.f;
    const float gd = g.grad_depth != nullptr ? g.grad_depth[p] : 0.f;
    const float gwhite = a.white_bkgd ? gr0 + gr1 + gr2 : 0.f;          // rgb += 1 - sum_t w_t
    float run = 0.f;                                    // sum_{k>t} g w_k alpha_k Tk_k
    for (int t = T - 1; t >= 0; --t) {
        const float *src, *zsrc; float* dst;
        locate(t, src, zsrc, dst);
        float4 c = make_float4(0.f, 0.f, 0.f, 0.f);
        float z = 0.f;
        if (src != nullptr) { c = *reinterpret_cast<const float4*>(src); z = zsrc[0]; }
        const float Tk = s_T[t][tid];
        const float e = expf(-c.w), alpha = 1.f - e, tt = 1.f - alpha + 1e-10f;
        const float wgt = alpha * Tk;
        const float gw = g.grad_weights != nullptr ? g.grad_weights[(long long)p * T + t] : 0.f;
        const float gwt = gw + gd * z + (gr0 * c.x + gr1 * c.y + gr2 * c.z) - gwhite;
        const float galpha = gwt * Tk - run / tt;
        run += gwt * alpha * Tk;
        if (dst != nullptr) *reinterpret_cast<float4*>(dst) = make_float4(wgt * gr0, wgt * gr1, wgt * gr2, galpha * e);
    }
}
void launch_composite_layers_bwd(const CompositeLayersBwd& g, hipStream_t st) {
    const int nf = g.fwd.L * g.fwd.Ns;                  // launch_composite_layers' branch
    const unsigned grid = (unsigned)cdiv(g.fwd.H * g.fwd.W, 256);
    if (nf <= 2) ENERF_LAUNCH_SIMPLE(k_composite_layers_bwd<2>, grid, 256, 0, st, g);
    else if (nf <= 4) ENERF_LAUNCH_SIMPLE(k_composite_layers_bwd<4>, grid, 256, 0, st, g);
    else if (nf <= 8) ENERF_LAUNCH_SIMPLE(k_composite_layers_bwd<8>, grid, 256, 0, st, g);
    else ENERF_LAUNCH_SIMPLE(k_composite_layers_bwd<16>, grid, 256, 0, st, g);
}

}  // namespace enerf
