// perceptual_vgg.h — the trainer's perceptual term (lib/train/losses/vgg_perceptual_loss.py:21-37 as losses/enerf.py:30-51 calls it:
// resize=False, feature_layers=[0,1,2,3], no style layers), forward and backward, on the device.  Included by io.hip after
// lpips_vgg.h, whose kernel it reuses.
//
//   x            (img - mean) / std per channel, the ImageNet mean / std
//   trunk        torchvision VGG16 features[:23]: the first ten convolutions of lpips_vgg.h's trunk (kVggSpec[0..9])
//   loss         sum_l mean|x_l - y_l| over the activations after relu1_2, relu2_2, relu3_3, relu4_3 (mean over N*C*H*W)
//
// Forward: k_vgg_conv3x3 as the evaluator runs it (pred and gt as ONE batch of 2N images, pool on load, blocked summation), with
// one more front for conv 0 (kVggStagePerceptual); every layer's output stays in the workspace.  The taps sum |x - y| in float64,
// one partial per block, added in a fixed order.
// Backward: the VGG weights are frozen, so it is ten data-gradient launches, conv 9 down to conv 0.  The gradient of a 3x3 / s1 /
// p1 convolution with respect to its input is the same convolution with the weights transposed in (cin, cout) and flipped in the
// taps: k_vgg_conv3x3 again on a second packed image per layer (k_vgg_dgrad_pack).  Everything elementwise — the ReLU mask
// (act > 0), the L1 taps' seeds sign(x - y) / count and the routing through the max pools' arg-max — happens while the kernel
// stages its tile (vgg_stage_dgrad): no masked or un-pooled gradient tensor is ever written.  The last layer (64 -> 3) is 1,728
// multiply-adds per pixel and has its own small kernel, which also divides by std and applies the upstream scalar.
//
// Workspace (floats from its start; perc_layout):  tap partials (4 x kLpipsTapBlocks doubles) | act_0 .. act_9, each (2N, H_i, W_i,
// C_i) channels-last with the N pred images first | two ping-pong gradient buffers.
#pragma once

namespace enerf {

constexpr int kPercLayers = 10;

struct PercLayout {
    int H[kPercLayers], W[kPercLayers];
    long long act[kPercLayers];        // float offsets of the saved activations
    long long grad[2];                 // grad[i & 1]: the output of data-gradient launch i (the gradient of conv i's input)
    long long floats;
};
PercLayout perc_layout(int N, int h, int w) {
    PercLayout L;
    long long o = (long long)4 * kLpipsTapBlocks * 2, g[2] = {0, 0};
    int H = h, W = w;
    for (int i = 0; i < kPercLayers; ++i) {
        if (kVggSpec[i].pool) { H /= 2; W /= 2; }
        L.H[i] = H; L.W[i] = W; L.act[i] = o;
        o += 2LL * N * H * W * kVggSpec[i].cout;
        if (i > 0) {
            const long long n = (long long)N * H * W * kVggSpec[i].cin;
            if (n > g[i & 1]) g[i & 1] = n;
        }
    }
    L.grad[0] = o; L.grad[1] = o + g[0];
    L.floats = o + g[0] + g[1];
    return L;
}
size_t perceptual_workspace_bytes(int N, int h, int w) { return (size_t)perc_layout(N, h, w).floats * sizeof(float); }
void perceptual_layout(int N, int h, int w, long long* offsets) {
    const PercLayout L = perc_layout(N, h, w);
    for (int i = 0; i < kPercLayers; ++i) offsets[i] = L.act[i];
}

// ---- packed image: forward layers (A operands | bias, as lpips_layer_offset lays them out) | data-gradient images ----
// data-gradient image of forward layer (cin, cout): conv 0 (cin = 3) the small kernel's [tap][3][64], else 9 * cout * cin A operands
long long vgg_dgrad_packed_floats(int cin, int cout) { return 9LL * cin * cout; }
bool vgg_dgrad_supported(int cin, int cout) {
    for (int i = 0; i < kPercLayers; ++i)
        if (kVggSpec[i].cin == cin && kVggSpec[i].cout == cout) return true;
    return false;
}
long long perc_dgrad_offset(int layer) {
    long long o = lpips_layer_offset(kPercLayers);
    for (int i = 0; i < layer; ++i) o += vgg_dgrad_packed_floats(kVggSpec[i].cin, kVggSpec[i].cout);
    return o;
}
long long perceptual_packed_floats() { return perc_dgrad_offset(kPercLayers); }

// w (cout, cin, 3, 3) of the forward layer -> the A operands of its data gradient, a convolution from cout to cin channels with
// wd[co' = ci][ci' = co][tap] = w[co][ci][8 - tap], in k_vgg_pack's order: packed[((tap*KS + ks)*RT + rt)*64 + lane], lane = (g, i):
// wd[co' = 16rt + i][ci' = 16cb + 4g + r][tap], ks = 4cb + r.  cin = 3: packed[(tap*3 + co')*64 + ci'] for k_vgg_dgrad3.
__global__ __launch_bounds__(256) void k_vgg_dgrad_pack(const float* __restrict__ w, int cin, int cout, float* __restrict__ packed) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 9LL * cin * cout) return;
    if (cin == 3) {
        const int cid = (int)(i & 63), cod = (int)((i >> 6) % 3), tap = (int)(i / 192);
        packed[i] = w[((long long)cid * 3 + cod) * 9 + (8 - tap)];
        return;
    }
    const int KS = cout / 4, RT = cin / 16, lane = (int)(i & 63);
    long long q = i >> 6;
    const int rt = (int)(q % RT); q /= RT;
    const int ks = (int)(q % KS), tap = (int)(q / KS);
    const int g = lane >> 4, cod = rt * 16 + (lane & 15), cb = ks >> 2, r = ks & 3, cid = cb * 16 + g * 4 + r;
    packed[i] = w[((long long)cid * cin + cod) * 9 + (8 - tap)];
}
void launch_vgg_dgrad_pack(const float* w, int cin, int cout, float* packed, hipStream_t st) {
    ENERF_LAUNCH_SIMPLE(k_vgg_dgrad_pack, (unsigned)cdivl(vgg_dgrad_packed_floats(cin, cout), 256), 256, 0, st, w, cin, cout, packed);
}
void launch_perceptual_pack(const enerf_perceptual_raw_t& raw, float* packed, hipStream_t st) {
    for (int i = 0; i < kPercLayers; ++i) {
        launch_vgg_conv3x3_pack(raw.conv[i].w, raw.conv[i].b, kVggSpec[i].cin, kVggSpec[i].cout, packed + lpips_layer_offset(i), st);
        launch_vgg_dgrad_pack(raw.conv[i].w, kVggSpec[i].cin, kVggSpec[i].cout, packed + perc_dgrad_offset(i), st);
    }
}

// ---- the last data gradient, 64 -> 3 -------------------------------------------------------------------------------------------
// 16 lanes per pixel (lane j: channels 4j .. 4j + 3 of the nine neighbours), 16 pixels per block; the 16 partial sums are added by
// a fixed xor tree.  g (N, H, W, 64); act (the ReLU mask, act > 0) or nullptr; out (N, H*W, 3) = sum * inv_std[c] (* *scale).
struct VggDgrad3Args {
    const float* wd;        // [tap][3][64]
    const float* g;
    const float* act;
    const float* scale;     // device scalar or nullptr (= 1)
    float* out;
    int N, H, W;
    float std[3];           // out = sum / std
};
__device__ __forceinline__ float row16_sumf(float v) {
    v += __shfl_xor(v, 8); v += __shfl_xor(v, 4); v += __shfl_xor(v, 2); v += __shfl_xor(v, 1);
    return v;
}
__global__ __launch_bounds__(256) void k_vgg_dgrad3(const VggDgrad3Args a) {
    __shared__ float4 wl[27 * 16];
    const int tid = threadIdx.x, row = tid >> 4, j = tid & 15;
    for (int i = tid; i < 27 * 16; i += 256) wl[i] = reinterpret_cast<const float4*>(a.wd)[i];
    __syncthreads();
    const long long P = (long long)a.N * a.H * a.W, p = (long long)blockIdx.x * 16 + row, pc = p < P ? p : P - 1;
    const int x = (int)(pc % a.W), y = (int)((pc / a.W) % a.H);
    const long long n = pc / ((long long)a.W * a.H);
    float s0 = 0.f, s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
        const int iy = y + tap / 3 - 1, ix = x + tap % 3 - 1;
        float4 gv = make_float4(0.f, 0.f, 0.f, 0.f);
        if (iy >= 0 && iy < a.H && ix >= 0 && ix < a.W) {
            const long long off = (((n * a.H + iy) * a.W + ix) * 64) + 4 * j;
            gv = *reinterpret_cast<const float4*>(a.g + off);
            if (a.act != nullptr) {
                const float4 av = *reinterpret_cast<const float4*>(a.act + off);
                gv = make_float4(av.x > 0.f ? gv.x : 0.f, av.y > 0.f ? gv.y : 0.f, av.z > 0.f ? gv.z : 0.f, av.w > 0.f ? gv.w : 0.f);
            }
        }
        const float4 w0 = wl[(tap * 3 + 0) * 16 + j], w1 = wl[(tap * 3 + 1) * 16 + j], w2 = wl[(tap * 3 + 2) * 16 + j];
        s0 += (gv.x * w0.x + gv.y * w0.y) + (gv.z * w0.z + gv.w * w0.w);
        s1 += (gv.x * w1.x + gv.y * w1.y) + (gv.z * w1.z + gv.w * w1.w);
        s2 += (gv.x * w2.x + gv.y * w2.y) + (gv.z * w2.z + gv.w * w2.w);
    }
    s0 = row16_sumf(s0); s1 = row16_sumf(s1); s2 = row16_sumf(s2);
    if (j != 0 || p >= P) return;
    float v0 = s0 / a.std[0], v1 = s1 / a.std[1], v2 = s2 / a.std[2];
    if (a.scale != nullptr) {
        const float sc = *a.scale;
        v0 *= sc; v1 *= sc; v2 *= sc;
    }
    float* o = a.out + p * 3;
    o[0] = v0; o[1] = v1; o[2] = v2;
}
void launch_vgg_dgrad3(const float* wd, const float* g, const float* act, const float* scale, float* out, int N, int H, int W,
                       bool by_std, hipStream_t st) {
    VggDgrad3Args a = {wd, g, act, scale, out, N, H, W, {1.f, 1.f, 1.f}};
    if (by_std) { a.std[0] = 0.229f; a.std[1] = 0.224f; a.std[2] = 0.225f; }
    ENERF_LAUNCH(k_vgg_dgrad3, (unsigned)cdivl((long long)N * H * W, 16), 256, 0, st, a);
}

// one data-gradient layer of forward layer (cin, cout): gout (N, H, W, cout) -> gin (N, H, W, cin); d.act == nullptr: plain
void launch_vgg_dgrad(const float* packed_d, int cin, int cout, const float* gout, float* gin, int N, int H, int W,
                      const VggDgradStage& d, hipStream_t st) {
    VggConvArgs a = {packed_d, gout, gin, cout, cin, H, W, H, W, 0, 0, cdiv(W, kVggTW), VggFront{}, d};
    const dim3 grid((unsigned)(a.tiles_x * cdiv(H, kVggTH)), (unsigned)(cin / 64), (unsigned)N);
    ENERF_LAUNCH((k_vgg_conv3x3<16, kVggStageDgrad>), grid, 256, 0, st, a);
}
void launch_vgg_conv3x3_dgrad(const float* packed_d, int cin, int cout, const float* gout, float* gin, int N, int H, int W,
                              hipStream_t st) {
    if (cin == 3) launch_vgg_dgrad3(packed_d, gout, nullptr, nullptr, gin, N, H, W, false, st);
    else launch_vgg_dgrad(packed_d, cin, cout, gout, gin, N, H, W, VggDgradStage{}, st);
}

// ---- the L1 taps ---------------------------------------------------------------------------------------------------------------
// feat (2N, P, C) as n4 float4 per half: sum |x - y| in float64 (the difference of two floats is exact there), one partial per block
__global__ __launch_bounds__(256) void k_perc_tap(const float* __restrict__ feat, long long n4, double* __restrict__ partial) {
    __shared__ double wsum[4];
    const int tid = threadIdx.x;
    const float4* x = reinterpret_cast<const float4*>(feat);
    const float4* y = x + n4;
    double acc = 0.0;
    for (long long i = (long long)blockIdx.x * 256 + tid; i < n4; i += (long long)gridDim.x * 256) {
        const float4 u = x[i], v = y[i];
        acc += (fabs((double)u.x - (double)v.x) + fabs((double)u.y - (double)v.y)) + (fabs((double)u.z - (double)v.z) + fabs((double)u.w - (double)v.w));
    }
    acc = wave_sum(acc);
    if ((tid & 63) == 0) wsum[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) partial[blockIdx.x] = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
}
struct PercFinishArgs { int nblk[4]; double count[4]; };
// one block: every tap's partials in a fixed order, l = sum / count, out = {((l0 + l1) + l2) + l3, l0 .. l3}
__global__ __launch_bounds__(256) void k_perc_finish(const double* __restrict__ partial, const PercFinishArgs f, double* __restrict__ out) {
    __shared__ double wsum[4][4];
    const int tid = threadIdx.x;
    for (int l = 0; l < 4; ++l) {
        double a = 0.0;
        for (int i = tid; i < f.nblk[l]; i += 256) a += partial[(long long)l * kLpipsTapBlocks + i];
        a = wave_sum(a);
        if ((tid & 63) == 0) wsum[l][tid >> 6] = a;
    }
    __syncthreads();
    if (tid != 0) return;
    double total = 0.0;
    for (int l = 0; l < 4; ++l) {
        const double d = ((wsum[l][0] + wsum[l][1]) + (wsum[l][2] + wsum[l][3])) / f.count[l];
        out[1 + l] = d;
        total = l == 0 ? d : total + d;
    }
    out[0] = total;
}

// pred / gt (N, h*w, 3) -> out {loss, l_0 .. l_3}; leaves act_0 .. act_9 in the workspace for launch_perceptual_bwd
void launch_perceptual_fwd(const float* packed, const float* pred, const float* gt, int N, int h, int w, void* workspace, double* out,
                           hipStream_t st) {
    const PercLayout L = perc_layout(N, h, w);
    float* ws = (float*)workspace;
    double* partial = (double*)workspace;
    PercFinishArgs fin;
    for (int i = 0; i < kPercLayers; ++i) {
        const VggLayerSpec& S = kVggSpec[i];
        VggConvArgs a = {packed + lpips_layer_offset(i), i == 0 ? nullptr : ws + L.act[i - 1], ws + L.act[i], S.cin, S.cout, L.H[i], L.W[i],
                         i == 0 ? h : L.H[i - 1], i == 0 ? w : L.W[i - 1], S.pool, 1, cdiv(L.W[i], kVggTW), VggFront{}, VggDgradStage{}};
        const dim3 grid((unsigned)(a.tiles_x * cdiv(L.H[i], kVggTH)), (unsigned)(S.cout / 64), (unsigned)(2 * N));
        if (i == 0) {
            a.f.pred = pred; a.f.gt = gt; a.f.B = N;
            ENERF_LAUNCH((k_vgg_conv3x3<4, kVggStagePerceptual>), grid, 256, 0, st, a);
        } else {
            ENERF_LAUNCH(k_vgg_conv3x3<16>, grid, 256, 0, st, a);
        }
        if (S.tap >= 0) {
            const long long n4 = (long long)N * L.H[i] * L.W[i] * S.cout / 4;
            const int nblk = (int)(cdivl(n4, 256) < kLpipsTapBlocks ? cdivl(n4, 256) : kLpipsTapBlocks);
            fin.nblk[S.tap] = nblk;
            fin.count[S.tap] = (double)(n4 * 4);
            ENERF_LAUNCH(k_perc_tap, (unsigned)nblk, 256, 0, st, (const float*)(ws + L.act[i]), n4, partial + (size_t)S.tap * kLpipsTapBlocks);
        }
    }
    ENERF_LAUNCH(k_perc_finish, 1u, 256, 0, st, (const double*)partial, fin, out);
}

// reads only the workspace launch_perceptual_fwd left and `packed`; grad_pred (N, h*w, 3) = d loss / d pred (* *grad_scale)
void launch_perceptual_bwd(const float* packed, int N, int h, int w, void* workspace, const float* grad_scale, float* grad_pred,
                           hipStream_t st) {
    const PercLayout L = perc_layout(N, h, w);
    float* ws = (float*)workspace;
    for (int i = kPercLayers - 1; i >= 1; --i) {
        const VggLayerSpec& S = kVggSpec[i];
        const long long half = (long long)N * L.H[i] * L.W[i] * S.cout;
        VggDgradStage d = {ws + L.act[i], S.tap >= 0 ? ws + L.act[i] + half : nullptr, (float)(1.0 / (double)half), 0, 0, 0};
        const float* gin = nullptr;
        if (i + 1 < kPercLayers) {
            gin = ws + L.grad[(i + 1) & 1];
            d.route = kVggSpec[i + 1].pool; d.gH = L.H[i + 1]; d.gW = L.W[i + 1];
        }
        launch_vgg_dgrad(packed + perc_dgrad_offset(i), S.cin, S.cout, gin, ws + L.grad[i & 1], N, L.H[i], L.W[i], d, st);
    }
    launch_vgg_dgrad3(packed + perc_dgrad_offset(0), ws + L.grad[1], ws + L.act[0], grad_scale, grad_pred, N, h, w, true, st);
}

}  // namespace enerf
