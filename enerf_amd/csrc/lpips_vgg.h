// lpips_vgg.h — the evaluators' third number, LPIPS (lib/evaluators/enerf.py:81-87, enerf_human.py:71-77:
// lpips.LPIPS(net='vgg'), lpips=True, spatial=False, eval mode), on the device.  Included by io.hip only (it uses that file's
// mask / rectangle helpers and wave_sum).
//
//   scaling layer  x = (in - shift) / scale per channel, in = (image - 0.5) * 2 with the pixels whose mask is off set to 0 first
//   trunk          torchvision VGG16 `features`: thirteen 3x3 / stride 1 / zero padding 1 convolutions with bias + ReLU, a 2x2 /
//                  stride 2 / floor max pool in front of convs 5, 10, 17, 24
//   taps           after relu1_2, relu2_2, relu3_3, relu4_3, relu5_3 (C = 64, 128, 256, 512, 512):
//                  d_l = mean over pixels of sum_c lin_l[c] * (f0 / (|f0| + 1e-10) - f1 / (|f1| + 1e-10))^2;  lpips = sum_l d_l
//
// k_vgg_conv3x3: implicit GEMM on v_mfma_f32_16x16x4_f32, D[cout][pixel] += W[cout][k] * X[k][pixel], the scheme of k_conv2d
// (conv2d.hip) with wide channels.  Activations are channels-last (N, H, W, C), N = 2B: pred images first, then gt, through
// the same launches (one weight fetch serves both).  A 256-thread block makes 8 x 32 pixels x 64 output channels; a wave owns
// 4 rows x 16 columns of them = 4 pixel tiles x 4 cout tiles = 16 accumulators, so one ds_read_b128 (a pixel's 4 channels of
// this lane group: 4 k-steps) feeds 16 MFMAs and one weight dword 4 MFMAs.  The input tile of ONE 16-channel chunk with its
// halo (10 x 34 pixels x 64 B = 21,760 B) is staged per pass; the weights of the chunk (9 x 4 x 4 dwords per lane) are
// streamed per tap row from the packed image (k_conv2d_pack's order [tap][cin/4][cout/16][lane]), never held: the 512 -> 512
// image is 9.4 MB.  The 2x2 max pool is taken while staging (four loads instead of one): no pooled tensor is ever written.
// Pixel tiles that lie wholly outside the image are skipped (a wave-uniform test), so a 1x1 map costs one tile, not sixteen.
// (The same kernel serves the trainer's perceptual term, perceptual_vgg.h: its MODE template parameter selects what is staged.)
// Conv 0 (3 -> 64, channels padded to 4, one k-step per tap) stages the evaluator's (B, h*w, 3) images directly: mask
// zeroing, rectangle offset, (x - 0.5) * 2 and the scaling layer on load — NOT folded into the bias: the zero padding comes
// after the scaling layer, so the halo is staged as zeros of the SCALED image.
#pragma once

namespace enerf {

constexpr int kVggTH = 8, kVggTW = 32, kVggIH = kVggTH + 2, kVggIW = kVggTW + 2, kVggNPX = kVggIH * kVggIW;
constexpr int kLpipsTapBlocks = 1024;      // partial sums per (tap, image): the tap kernel's largest grid

__host__ __device__ __forceinline__ int vgg_cinp(int cin) { return cin < 4 ? 4 : cin; }
long long vgg_conv3x3_packed_floats(int cin, int cout) { return 9LL * vgg_cinp(cin) * cout + cout; }     // A operands | bias
bool vgg_conv3x3_supported(int cin, int cout) {
    for (int i = 0; i < kVggLayers; ++i)
        if (kVggSpec[i].cin == cin && kVggSpec[i].cout == cout) return true;
    return false;
}
long long lpips_layer_offset(int layer) {
    long long o = 0;
    for (int i = 0; i < layer; ++i) o += vgg_conv3x3_packed_floats(kVggSpec[i].cin, kVggSpec[i].cout);
    return o;
}
long long lpips_lin_offset(int tap) {
    long long o = lpips_layer_offset(kVggLayers);
    for (int l = 0; l < tap; ++l) o += kLpipsTapC[l];
    return o;
}
long long lpips_packed_floats() { return lpips_lin_offset(5); }

// packed[((tap*KS + ks)*RT + rt)*64 + lane], lane = (g, i): w[cout = 16rt + i][cin = 16cb + 4g + r][tap], ks = 4cb + r (Cin = 3:
// ks = 0, cin = g, the fourth channel 0); then the bias
__global__ __launch_bounds__(256) void k_vgg_pack(const float* __restrict__ w, const float* __restrict__ bias, int cin, int cout,
                                                  float* __restrict__ packed) {
    const int cinp = vgg_cinp(cin), CPL = cinp >= 16 ? 4 : 1, KS = cinp / 4, RT = cout / 16;
    const long long nw = 9LL * KS * RT * 64;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nw + cout) return;
    if (i >= nw) { packed[i] = bias[i - nw]; return; }
    const int lane = (int)(i & 63);
    long long q = i >> 6;
    const int rt = (int)(q % RT); q /= RT;
    const int ks = (int)(q % KS), tap = (int)(q / KS);
    const int g = lane >> 4, co = rt * 16 + (lane & 15);
    const int cb = ks / CPL, r = ks - cb * CPL;
    const int ci = cb * 4 * CPL + g * CPL + r;
    packed[i] = ci < cin ? w[((long long)co * cin + ci) * 9 + tap] : 0.f;
}
void launch_vgg_conv3x3_pack(const float* w, const float* bias, int cin, int cout, float* packed, hipStream_t st) {
    ENERF_LAUNCH_SIMPLE(k_vgg_pack, (unsigned)cdivl(vgg_conv3x3_packed_floats(cin, cout), 256), 256, 0, st, w, bias, cin, cout, packed);
}
__global__ __launch_bounds__(256) void k_lpips_copy_lin(const float* __restrict__ lin, int n, float* __restrict__ dst) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = lin[i];
}
void launch_lpips_pack(const enerf_lpips_raw_t& raw, float* packed, hipStream_t st) {
    for (int i = 0; i < kVggLayers; ++i)
        launch_vgg_conv3x3_pack(raw.conv[i].w, raw.conv[i].b, kVggSpec[i].cin, kVggSpec[i].cout, packed + lpips_layer_offset(i), st);
    for (int l = 0; l < 5; ++l)
        ENERF_LAUNCH_SIMPLE(k_lpips_copy_lin, (unsigned)cdiv(kLpipsTapC[l], 256), 256, 0, st, raw.lin[l], kLpipsTapC[l],
                            packed + lpips_lin_offset(l));
}

// what k_vgg_conv3x3 stages (its MODE): the trunk's own input (the evaluator front when f.pred is set), the trainer's images
// through the perceptual term's normalisation, or the masked / seeded / pool-routed gradient of a data-gradient layer
// (perceptual_vgg.h); the arithmetic behind the staging is one and the same
constexpr int kVggStageTrunk = 0, kVggStagePerceptual = 1, kVggStageDgrad = 2;
struct VggDgradStage {
    const float* act;       // (N, H, W, cin) the layer's saved forward output: ReLU mask (and pool arg-max); nullptr: `in` as it is
    const float* act_gt;    // the same of the gt images on a tap layer (the seed sign(act - act_gt) * seed), else nullptr
    float seed;             // 1 / (N * cin * H * W)
    int route, gH, gW;      // route: `in` is (N, gH, gW, cin), the gradient of the 2x2 floor max pool of `act`
};
struct VggConvArgs {
    const float* wpk;       // the layer's packed image (A operands | bias; no bias in MODE kVggStageDgrad)
    const float* in;        // (N, Hin, Win, cin) channels-last; unused by the fronts
    float* out;             // (N, H, W, cout)
    int cin, cout, H, W, Hin, Win, pool, relu, tiles_x;
    VggFront f;             // f.pred != nullptr: conv 0 reads (B, h*w, 3) images (n < f.B: pred, else gt)
    VggDgradStage d;
};

// the trainer's images (lib/train/losses/vgg_perceptual_loss.py:18-26): (v - mean) / std on load; a.f.pred / a.f.gt (B, H*W, 3)
__device__ __forceinline__ float4 vgg_stage_perceptual(const VggConvArgs& a, int n, int gy, int gx) {
    const float* src = n < a.f.B ? a.f.pred : a.f.gt;
    const float* p = src + (((long long)(n < a.f.B ? n : n - a.f.B) * a.H + gy) * a.W + gx) * 3;
    return make_float4((p[0] - 0.485f) / 0.229f, (p[1] - 0.456f) / 0.224f, (p[2] - 0.406f) / 0.225f, 0.f);
}
// MaxPool2d(2, 2) backward: position k = 2 * (y & 1) + (x & 1) keeps the gradient when it holds the FIRST maximum of its window in
// row-major order (torch's return_indices rule)
__device__ __forceinline__ bool vgg_pool_first_max(int k, float v0, float v1, float v2, float v3) {
    int m = 0;
    float best = v0;
    if (v1 > best) { best = v1; m = 1; }
    if (v2 > best) { best = v2; m = 2; }
    if (v3 > best) { best = v3; m = 3; }
    return m == k;
}
__device__ __forceinline__ float vgg_sign_seed(float x, float y, float seed) { return x > y ? seed : (x < y ? -seed : 0.f); }
// the input of a data-gradient layer, four channels c .. c + 3 of pixel (gy, gx): the incoming gradient (routed through the pool's
// arg-max when the forward pooled on load behind this layer), plus the L1 tap's seed, times the ReLU mask (act > 0)
__device__ __forceinline__ float4 vgg_stage_dgrad(const VggConvArgs& a, int n, int gy, int gx, int c) {
    const long long rowf = (long long)a.W * a.cin, off = ((long long)n * a.H + gy) * rowf + (long long)gx * a.cin + c;
    if (a.d.act == nullptr) return *reinterpret_cast<const float4*>(a.in + off);
    const float4 av = *reinterpret_cast<const float4*>(a.d.act + off);
    float4 g = make_float4(0.f, 0.f, 0.f, 0.f);
    if (a.in != nullptr) {
        if (!a.d.route) {
            g = *reinterpret_cast<const float4*>(a.in + off);
        } else if ((gy >> 1) < a.d.gH && (gx >> 1) < a.d.gW) {           // rows / columns beyond the floor: 0
            const int py = gy >> 1, px = gx >> 1, k = 2 * (gy & 1) + (gx & 1);
            const float4 gi = *reinterpret_cast<const float4*>(a.in + (((long long)n * a.d.gH + py) * a.d.gW + px) * a.cin + c);
            const float* p = a.d.act + ((long long)n * a.H + 2 * py) * rowf + (long long)(2 * px) * a.cin + c;
            const float4 v0 = *reinterpret_cast<const float4*>(p), v1 = *reinterpret_cast<const float4*>(p + a.cin);
            const float4 v2 = *reinterpret_cast<const float4*>(p + rowf), v3 = *reinterpret_cast<const float4*>(p + rowf + a.cin);
            g = make_float4(vgg_pool_first_max(k, v0.x, v1.x, v2.x, v3.x) ? gi.x : 0.f, vgg_pool_first_max(k, v0.y, v1.y, v2.y, v3.y) ? gi.y : 0.f,
                            vgg_pool_first_max(k, v0.z, v1.z, v2.z, v3.z) ? gi.z : 0.f, vgg_pool_first_max(k, v0.w, v1.w, v2.w, v3.w) ? gi.w : 0.f);
        }
    }
    if (a.d.act_gt != nullptr) {
        const float4 yv = *reinterpret_cast<const float4*>(a.d.act_gt + off);
        g.x += vgg_sign_seed(av.x, yv.x, a.d.seed); g.y += vgg_sign_seed(av.y, yv.y, a.d.seed);
        g.z += vgg_sign_seed(av.z, yv.z, a.d.seed); g.w += vgg_sign_seed(av.w, yv.w, a.d.seed);
    }
    return make_float4(av.x > 0.f ? g.x : 0.f, av.y > 0.f ? g.y : 0.f, av.z > 0.f ? g.z : 0.f, av.w > 0.f ? g.w : 0.f);
}

// one staged item: four channels of the input pixel (gy, gx) of image n (inside the image; the caller zero-fills the rest)
template <int CB, int MODE>
__device__ __forceinline__ float4 vgg_stage_load(const VggConvArgs& a, int n, int gy, int gx, int cb, int q) {
    if (MODE == kVggStageDgrad) return vgg_stage_dgrad(a, n, gy, gx, cb * 16 + q * 4);
    if (MODE == kVggStagePerceptual) return vgg_stage_perceptual(a, n, gy, gx);
    if (CB == 16) {
        const long long rowf = (long long)a.Win * a.cin;
        if (!a.pool) return *reinterpret_cast<const float4*>(a.in + ((long long)n * a.Hin + gy) * rowf + (long long)gx * a.cin + cb * 16 + q * 4);
        // MaxPool2d(2, 2), floor mode: H = Hin / 2, so rows 2gy, 2gy + 1 and columns 2gx, 2gx + 1 all exist
        const float* p = a.in + ((long long)n * a.Hin + 2 * gy) * rowf + (long long)(2 * gx) * a.cin + cb * 16 + q * 4;
        const float4 v0 = *reinterpret_cast<const float4*>(p), v1 = *reinterpret_cast<const float4*>(p + a.cin);
        const float4 v2 = *reinterpret_cast<const float4*>(p + rowf), v3 = *reinterpret_cast<const float4*>(p + rowf + a.cin);
        return make_float4(fmaxf(fmaxf(v0.x, v1.x), fmaxf(v2.x, v3.x)), fmaxf(fmaxf(v0.y, v1.y), fmaxf(v2.y, v3.y)),
                           fmaxf(fmaxf(v0.z, v1.z), fmaxf(v2.z, v3.z)), fmaxf(fmaxf(v0.w, v1.w), fmaxf(v2.w, v3.w)));
    }
    if (a.f.pred == nullptr) {
        const float* p = a.in + (((long long)n * a.H + gy) * a.W + gx) * 3;
        return make_float4(p[0], p[1], p[2], 0.f);
    }
    // enerf.py:67-69 / enerf_human.py:55-56 (mask off -> 0), :82-83 / :72-73 ((x - 0.5) * 2), then lpips' ScalingLayer
    const int b = n < a.f.B ? n : n - a.f.B;
    const float* src = n < a.f.B ? a.f.pred : a.f.gt;
    const long long pix = ((long long)b * a.f.img_h + (a.f.y0 + gy)) * a.f.img_w + (a.f.x0 + gx);
    const bool on = a.f.mask == nullptr || ssim_mask_on(a.f.mask, a.f.mask_bytes, a.f.mask_mode, pix);
    const float r0 = src[pix * 3], r1 = src[pix * 3 + 1], r2 = src[pix * 3 + 2];
    const float x0 = ((on ? r0 : 0.f) - 0.5f) * 2.f, x1 = ((on ? r1 : 0.f) - 0.5f) * 2.f, x2 = ((on ? r2 : 0.f) - 0.5f) * 2.f;
    return make_float4((x0 - -0.030f) / 0.458f, (x1 - -0.088f) / 0.448f, (x2 - -0.188f) / 0.450f, 0.f);
}

// CB: input channels per LDS pass: 16 (cin a multiple of 16) or 4 (the 3-channel first layer).  grid (pixel tiles, cout / 64, N)
// The data-gradient staging (up to six loads per item) pushes the register count one past 256; its instantiation alone is told to
// stay at two waves per SIMD, like the trunk's (two blocks per CU: one stages while the other multiplies).  The trunk's own
// instantiations are compiled exactly as before.
#ifdef ENERF_EMU
#define ENERF_VGG_WAVES(mode)
#else
#define ENERF_VGG_WAVES(mode) __attribute__((amdgpu_waves_per_eu((mode) == kVggStageDgrad ? 2 : 1)))
#endif
template <int CB, int MODE = kVggStageTrunk>
__global__ __launch_bounds__(256) ENERF_VGG_WAVES(MODE) void k_vgg_conv3x3(const VggConvArgs a) {
    constexpr int CPL = CB / 4, QV = CB / 4, NIT = (kVggNPX * QV + 255) / 256;
    __shared__ float4 lds4[kVggNPX * QV];
    const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, j = lane & 15;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6), wy = wv >> 1, wx = wv & 1;
    const int tile = blockIdx.x, ty = tile / a.tiles_x, tx = tile - ty * a.tiles_x;
    const int cog = blockIdx.y, n = blockIdx.z;
    const int oy0 = ty * kVggTH, ox0 = tx * kVggTW;
    const int KS = vgg_cinp(a.cin) / 4, RT = a.cout / 16, NCB = KS / CPL;
    // wave-uniform: how many of this wave's pixel tiles (row oy0 + 4wy + c, columns ox0 + 16wx ..) reach into the image
    int nrow = a.H - (oy0 + 4 * wy);
    nrow = nrow > 4 ? 4 : nrow;
    if (ox0 + 16 * wx >= a.W) nrow = 0;

    // blocked summation: a pass (144 terms: 9 taps x 16 channels) accumulates from zero in `acc` and is then added to `sum`, so
    // the rounding error of a 4608-term dot product grows with 144 + 32, not with 4608 (one extra add per 36 MFMAs)
    f32x4 acc[4][4], sum[4][4];
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int rt = 0; rt < 4; ++rt) sum[c][rt] = f32x4{0.f, 0.f, 0.f, 0.f};

#pragma unroll 1
    for (int cb = 0; cb < NCB; ++cb) {
        if (cb > 0) __syncthreads();
        float4 sv[NIT];
#pragma unroll
        for (int it = 0; it < NIT; ++it) {                      // the loads of a pass are independent: all in flight together
            const int i = it * 256 + tid, ic = i < kVggNPX * QV ? i : kVggNPX * QV - 1;
            const int px = ic / QV, q = ic - px * QV;
            const int ly = px / kVggIW, lx = px - ly * kVggIW, gy = oy0 - 1 + ly, gx = ox0 - 1 + lx;
            sv[it] = make_float4(0.f, 0.f, 0.f, 0.f);           // zero padding (of the scaled image for conv 0) and tile overhang
            if (gy >= 0 && gy < a.H && gx >= 0 && gx < a.W) sv[it] = vgg_stage_load<CB, MODE>(a, n, gy, gx, cb, q);
        }
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int i = it * 256 + tid;
            if (i < kVggNPX * QV) lds4[i] = sv[it];
        }
        __syncthreads();
        if (nrow <= 0) continue;
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int rt = 0; rt < 4; ++rt) acc[c][rt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
        for (int kh = 0; kh < 3; ++kh) {
            // this tap row's A operands: 3 taps x CPL k-steps x 4 cout tiles, one coalesced dword per lane each
            float aq[3 * CPL * 4];
            const float* wt = a.wpk + lane + ((long long)(kh * 3) * KS + cb * CPL) * RT * 64 + cog * 4 * 64;
#pragma unroll
            for (int kw = 0; kw < 3; ++kw)
#pragma unroll
                for (int r = 0; r < CPL; ++r)
#pragma unroll
                    for (int rt = 0; rt < 4; ++rt) aq[(kw * CPL + r) * 4 + rt] = wt[((long long)(kw * KS + r) * RT + rt) * 64];
#pragma unroll
            for (int kw = 0; kw < 3; ++kw)
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    if (c >= nrow) continue;
                    const int px = (4 * wy + c + kh) * kVggIW + 16 * wx + j + kw;
                    float bv[4];
                    if (CB == 16) {
                        const float4 t = lds4[px * QV + g];
                        bv[0] = t.x; bv[1] = t.y; bv[2] = t.z; bv[3] = t.w;
                    } else {
                        bv[0] = reinterpret_cast<const float*>(lds4)[px * 4 + g];
                    }
#pragma unroll
                    for (int r = 0; r < CPL; ++r)
#pragma unroll
                        for (int rt = 0; rt < 4; ++rt)
                            acc[c][rt] = __builtin_amdgcn_mfma_f32_16x16x4f32(aq[(kw * CPL + r) * 4 + rt], bv[r], acc[c][rt], 0, 0, 0);
                }
        }
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int rt = 0; rt < 4; ++rt) sum[c][rt] += acc[c][rt];
    }

    // epilogue: bias, ReLU (a data gradient has neither); lane (g, j) holds channels 64cog + 16rt + 4g .. + 3 of pixel j of each of its tiles
    const float* bias = a.wpk + 9LL * KS * RT * 64;
    const int ox = ox0 + 16 * wx + j;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int oy = oy0 + 4 * wy + c;
        if (c >= nrow || ox >= a.W) continue;
        float* op = a.out + (((long long)n * a.H + oy) * a.W + ox) * a.cout;
#pragma unroll
        for (int rt = 0; rt < 4; ++rt) {
            const int co = cog * 64 + rt * 16 + 4 * g;
            if (MODE == kVggStageDgrad) {
                *reinterpret_cast<float4*>(op + co) = make_float4(sum[c][rt][0], sum[c][rt][1], sum[c][rt][2], sum[c][rt][3]);
                continue;
            }
            const float4 bq = *reinterpret_cast<const float4*>(bias + co);
            float4 v = make_float4(sum[c][rt][0] + bq.x, sum[c][rt][1] + bq.y, sum[c][rt][2] + bq.z, sum[c][rt][3] + bq.w);
            if (a.relu) v = make_float4(relu1(v.x), relu1(v.y), relu1(v.z), relu1(v.w));
            *reinterpret_cast<float4*>(op + co) = v;
        }
    }
}

// in: (N, Hin, Win, cin) channels-last, pooled 2x2 on load when `pool` (then H = Hin / 2, W = Win / 2), or nullptr with a front
void launch_vgg_conv3x3(const float* packed_layer, int cin, int cout, const float* in, float* out, int N, int H, int W, int pool,
                        int Hin, int Win, int relu, const VggFront* front, hipStream_t st) {
    VggConvArgs a = {packed_layer, in, out, cin, cout, H, W, Hin, Win, pool, relu, cdiv(W, kVggTW), VggFront{}};
    if (front != nullptr) a.f = *front;
    const dim3 grid((unsigned)(a.tiles_x * cdiv(H, kVggTH)), (unsigned)(cout / 64), (unsigned)N);
    if (cin == 3) ENERF_LAUNCH(k_vgg_conv3x3<4>, grid, 256, 0, st, a);
    else ENERF_LAUNCH(k_vgg_conv3x3<16>, grid, 256, 0, st, a);
}

// ---- the tap: both images' features of one slice -> one float64 partial per block ------------------------------------------------
// 16 lanes per pixel (a row of the wave), 16 pixels per block and step; the channel sums, the normalised difference and the pixel sum
// are all float64 (the features are fp32: their squares and the products with lin are exact).  Divisions, not reciprocals, and no
// contraction: identical features give a difference of exactly 0.
__device__ __forceinline__ double row16_sum(double v) {
    v += __shfl_xor(v, 8); v += __shfl_xor(v, 4); v += __shfl_xor(v, 2); v += __shfl_xor(v, 1);
    return v;
}
__device__ __forceinline__ double lpips_term(double lin, double u, double den_u, double v, double den_v) {
#ifndef ENERF_EMU
#pragma clang fp contract(off)
#endif
    const double nu = u / den_u, nv = v / den_v, e = nu - nv;
    return lin * (e * e);
}
// grid (blocks, B); feat (2B, P, C): image b and image B + b; partial (B, kLpipsTapBlocks) of this tap
__global__ __launch_bounds__(256) void k_lpips_tap(const float* __restrict__ feat, const float* __restrict__ lin, int B, int C,
                                                   long long P, double* __restrict__ partial) {
    __shared__ double wsum[4];
    const int tid = threadIdx.x, row = tid >> 4, j = tid & 15, b = blockIdx.y, C4 = C / 4;
    const float* f0 = feat + (long long)b * P * C;
    const float* f1 = feat + (long long)(B + b) * P * C;
    double acc = 0.0;
    for (long long base = (long long)blockIdx.x * 16; base < P; base += (long long)gridDim.x * 16) {     // block-uniform trip count
        const long long p = base + row, pc = p < P ? p : P - 1;
        const float4* a0 = reinterpret_cast<const float4*>(f0 + pc * C);
        const float4* a1 = reinterpret_cast<const float4*>(f1 + pc * C);
        double s0 = 0.0, s1 = 0.0;
        for (int q = j; q < C4; q += 16) {
            const float4 u = a0[q], v = a1[q];
            s0 += ((double)u.x * u.x + (double)u.y * u.y) + ((double)u.z * u.z + (double)u.w * u.w);
            s1 += ((double)v.x * v.x + (double)v.y * v.y) + ((double)v.z * v.z + (double)v.w * v.w);
        }
        s0 = row16_sum(s0);
        s1 = row16_sum(s1);
        const double d0 = sqrt(s0) + 1e-10, d1 = sqrt(s1) + 1e-10;
        double d = 0.0;
        for (int q = j; q < C4; q += 16) {
            const float4 u = a0[q], v = a1[q], l = reinterpret_cast<const float4*>(lin)[q];
            d += (lpips_term(l.x, u.x, d0, v.x, d1) + lpips_term(l.y, u.y, d0, v.y, d1)) +
                 (lpips_term(l.z, u.z, d0, v.z, d1) + lpips_term(l.w, u.w, d0, v.w, d1));
        }
        d = row16_sum(d);
        if (j == 0 && p < P) acc += d;
    }
    acc = wave_sum(acc);
    if ((tid & 63) == 0) wsum[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) partial[(long long)b * kLpipsTapBlocks + blockIdx.x] = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
}

struct LpipsFinishArgs { int nblk[5]; double pixels[5]; };
// one block per image: every tap's partials in a fixed order, d_l = sum / pixels, out[b] = {(((d0 + d1) + d2) + d3) + d4, d0 .. d4}
__global__ __launch_bounds__(256) void k_lpips_finish(const double* __restrict__ partial, int B, const LpipsFinishArgs f,
                                                      double* __restrict__ out) {
    __shared__ double wsum[5][4];
    const int tid = threadIdx.x, b = blockIdx.x;
    for (int l = 0; l < 5; ++l) {
        double a = 0.0;
        for (int i = tid; i < f.nblk[l]; i += 256) a += partial[((long long)l * B + b) * kLpipsTapBlocks + i];
        a = wave_sum(a);
        if ((tid & 63) == 0) wsum[l][tid >> 6] = a;
    }
    __syncthreads();
    if (tid != 0) return;
    double total = 0.0;
    for (int l = 0; l < 5; ++l) {
        const double d = ((wsum[l][0] + wsum[l][1]) + (wsum[l][2] + wsum[l][3])) / f.pixels[l];
        out[b * 6 + 1 + l] = d;
        total = l == 0 ? d : total + d;
    }
    out[b * 6] = total;
}

// workspace: tap partials (5, B, kLpipsTapBlocks) double | activations A | activations B, each (2B, rh, rw, 64) floats (the
// largest layer; the deeper ones are smaller)
size_t eval_lpips_workspace_bytes(int B, int rh, int rw) {
    return (size_t)5 * B * kLpipsTapBlocks * sizeof(double) + 2 * ((size_t)2 * B * rh * rw * 64 * sizeof(float));
}
void launch_eval_lpips(const float* packed, const VggFront& front, int rh, int rw, void* workspace, double* out, hipStream_t st) {
    const int B = front.B, N = 2 * B;
    double* partial = (double*)workspace;
    float* act[2];
    act[0] = (float*)((char*)workspace + (size_t)5 * B * kLpipsTapBlocks * sizeof(double));
    act[1] = act[0] + (size_t)N * rh * rw * 64;
    LpipsFinishArgs fin;
    int H = rh, W = rw, cur = 0;                          // cur: the buffer the previous layer wrote
    for (int i = 0; i < kVggLayers; ++i) {
        const VggLayerSpec& L = kVggSpec[i];
        const int Hin = H, Win = W;
        if (L.pool) { H /= 2; W /= 2; }
        const int dst = i == 0 ? 0 : cur ^ 1;
        launch_vgg_conv3x3(packed + lpips_layer_offset(i), L.cin, L.cout, i == 0 ? nullptr : act[cur], act[dst], N, H, W, L.pool,
                           Hin, Win, 1, i == 0 ? &front : nullptr, st);
        cur = dst;
        if (L.tap >= 0) {
            const long long P = (long long)H * W;
            const int nblk = (int)(cdivl(P, 16) < kLpipsTapBlocks ? cdivl(P, 16) : kLpipsTapBlocks);
            fin.nblk[L.tap] = nblk;
            fin.pixels[L.tap] = (double)P;
            ENERF_LAUNCH(k_lpips_tap, dim3((unsigned)nblk, (unsigned)B), 256, 0, st, (const float*)act[cur],
                         packed + lpips_lin_offset(L.tap), B, L.cout, P, partial + (size_t)L.tap * B * kLpipsTapBlocks);
        }
    }
    ENERF_LAUNCH(k_lpips_finish, (unsigned)B, 256, 0, st, (const double*)partial, B, fin, out);
}

// cv2.boundingRect (enerf_human.py:64) under its own entry: k_mask_bbox's encoded box rewritten in place as {x, y, w, h}
__global__ __launch_bounds__(64) void k_bbox_xywh(int* __restrict__ box, int B, int img_h, int img_w) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const SsimRect R = ssim_rect(2, img_h, img_w, 0, 0, box + b * 4);
    box[b * 4] = R.x0; box[b * 4 + 1] = R.y0; box[b * 4 + 2] = R.rw; box[b * 4 + 3] = R.rh;
}
void launch_mask_bbox(const void* mask, int mask_bytes, int mask_mode, int B, int img_h, int img_w, int* rect, hipStream_t st) {
    zero_async(rect, (size_t)B * 16, st);
    ENERF_LAUNCH(k_mask_bbox, dim3((unsigned)(img_h < 512 ? img_h : 512), (unsigned)B), 256, 0, st, (const unsigned char*)mask,
                 mask_bytes, mask_mode, img_h, img_w, rect);
    ENERF_LAUNCH_SIMPLE(k_bbox_xywh, (unsigned)cdiv(B, 64), 64, 0, st, rect, B, img_h, img_w);
}

}  // namespace enerf
