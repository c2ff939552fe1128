// io.hip — the steps either side of the rendering path, on device:
//   before: full-image ray generation (lib/datasets/enerf_utils.py:61-71, numpy on the host today; 10.5 MB of
//           rays_1 per 512x640 frame would otherwise cross PCIe every frame)
//   after:  uint8 packing + vertical flip for presentation (gui_human.py:88-91) and the evaluator's masked
//           PSNR / depth statistics (lib/evaluators/enerf.py:67-71, 88-103), SSIM (:76, enerf_human.py:54-66) and LPIPS (:81-87;
//           lpips_vgg.h, included at the end: the one MFMA kernel here) without a D2H copy of fp32 images.
// All HBM-bound, one thread per output element — except the SSIM kernels at the end (LDS tiles, float64 window sums).
#include "kernels.h"

namespace enerf {

// -------------------------------------------------------------------------------------------------
// rays[b][y*W+x] = [o(3) | d(3) | x | y],  o = c2w[:3,3],  d = c2w[:3,:3] · inv(K') · [x,y,1]^T,
// K' = K with rows 0,1 scaled by `scale`, c2w = inv(tar_ext).  The reference does this in float64 numpy
// and casts to float32 (enerf_utils.py:61-71); lane 0 of each block builds the 3x3 in fp64 in LDS.
// -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_gen_rays(const float* __restrict__ tar_ext, const float* __restrict__ tar_ixt,
                                                  int B, int Hr, int Wr, float scale, float* __restrict__ rays) {
    __shared__ double M[12];       // 3x3 (c2w_R · K'^-1) | origin(3)
    const long long npix = (long long)Hr * Wr;
    const int blocks_per_img = (int)cdivl(npix, 256);
    const int b = blockIdx.x / blocks_per_img;
    const long long p = (long long)(blockIdx.x - b * blocks_per_img) * 256 + threadIdx.x;
    if (threadIdx.x == 0) {
        double e[16], ei[16];
        for (int k = 0; k < 16; ++k) e[k] = (double)tar_ext[b * 16 + k];
        bool ok = inv4x4(e, ei);
        const float* K = tar_ixt + b * 9;
        // inverse of the scaled intrinsics (general 3x3, cofactors)
        double k[9];
        for (int i = 0; i < 9; ++i) k[i] = (double)K[i] * (i < 6 ? (double)scale : 1.0);
        double c00 = k[4] * k[8] - k[5] * k[7], c01 = k[5] * k[6] - k[3] * k[8], c02 = k[3] * k[7] - k[4] * k[6];
        double det = k[0] * c00 + k[1] * c01 + k[2] * c02;
        double ki[9] = {c00, k[2] * k[7] - k[1] * k[8], k[1] * k[5] - k[2] * k[4],
                        c01, k[0] * k[8] - k[2] * k[6], k[2] * k[3] - k[0] * k[5],
                        c02, k[1] * k[6] - k[0] * k[7], k[0] * k[4] - k[1] * k[3]};
        for (int i = 0; i < 9; ++i) ki[i] = (ok && det != 0.0) ? ki[i] / det : NAN;
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) {
                double a = 0;
                for (int t = 0; t < 3; ++t) a += ei[r * 4 + t] * ki[t * 3 + c];
                M[r * 3 + c] = a;
            }
        M[9] = ei[3]; M[10] = ei[7]; M[11] = ei[11];
    }
    __syncthreads();
    if (p >= npix) return;
    const int y = (int)(p / Wr), x = (int)(p - (long long)y * Wr);
    float* o = rays + ((long long)b * npix + p) * 8;
    const double fx = (double)x, fy = (double)y;
    const float4 a = make_float4((float)M[9], (float)M[10], (float)M[11], (float)(M[0] * fx + M[1] * fy + M[2]));
    const float4 c = make_float4((float)(M[3] * fx + M[4] * fy + M[5]), (float)(M[6] * fx + M[7] * fy + M[8]), (float)x,
                                 (float)y);
    *reinterpret_cast<float4*>(o) = a;
    *reinterpret_cast<float4*>(o + 4) = c;
}
void launch_gen_rays(const float* tar_ext, const float* tar_ixt, int B, int Hr, int Wr, float scale, float* rays,
                     hipStream_t st) {
    const unsigned grid = (unsigned)(cdivl((long long)Hr * Wr, 256) * B);
    ENERF_LAUNCH(k_gen_rays, grid, 256, 0, st, tar_ext, tar_ixt, B, Hr, Wr, scale, rays);
}

// -------------------------------------------------------------------------------------------------
// The training branch of build_rays (enerf_utils.py:33-56): the host RNG picks the pixel list (X, Y) exactly as the
// reference does (np.random permutation / randint / patches); the rays of those pixels are built here:
// rays[b][n] = [o | c2w_R · inv(K') · [X,Y,1]^T | X | Y].  Same fp64 3x3 as k_gen_rays.
// -------------------------------------------------------------------------------------------------
__device__ __forceinline__ void ray_matrix(const float* tar_ext, const float* tar_ixt, int b, float scale, double* M) {
    double e[16], ei[16];
    for (int k = 0; k < 16; ++k) e[k] = (double)tar_ext[b * 16 + k];
    bool ok = inv4x4(e, ei);
    const float* K = tar_ixt + b * 9;
    double k[9];
    for (int i = 0; i < 9; ++i) k[i] = (double)K[i] * (i < 6 ? (double)scale : 1.0);
    double c00 = k[4] * k[8] - k[5] * k[7], c01 = k[5] * k[6] - k[3] * k[8], c02 = k[3] * k[7] - k[4] * k[6];
    double det = k[0] * c00 + k[1] * c01 + k[2] * c02;
    double ki[9] = {c00, k[2] * k[7] - k[1] * k[8], k[1] * k[5] - k[2] * k[4],
                    c01, k[0] * k[8] - k[2] * k[6], k[2] * k[3] - k[0] * k[5],
                    c02, k[1] * k[6] - k[0] * k[7], k[0] * k[4] - k[1] * k[3]};
    for (int i = 0; i < 9; ++i) ki[i] = (ok && det != 0.0) ? ki[i] / det : NAN;
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) {
            double a = 0;
            for (int t = 0; t < 3; ++t) a += ei[r * 4 + t] * ki[t * 3 + c];
            M[r * 3 + c] = a;
        }
    M[9] = ei[3]; M[10] = ei[7]; M[11] = ei[11];
}
__global__ __launch_bounds__(256) void k_gen_rays_at(const float* __restrict__ tar_ext, const float* __restrict__ tar_ixt,
                                                     const int* __restrict__ xy, int B, int N, float scale,
                                                     float* __restrict__ rays) {
    __shared__ double M[12];
    const int blocks_per_b = cdiv(N, 256);
    const int b = blockIdx.x / blocks_per_b;
    const int n = (blockIdx.x - b * blocks_per_b) * 256 + threadIdx.x;
    if (threadIdx.x == 0) ray_matrix(tar_ext, tar_ixt, b, scale, M);
    __syncthreads();
    if (n >= N) return;
    const int x = xy[((long long)b * N + n) * 2], y = xy[((long long)b * N + n) * 2 + 1];
    const double fx = (double)x, fy = (double)y;
    float* o = rays + ((long long)b * N + n) * 8;
    *reinterpret_cast<float4*>(o) = make_float4((float)M[9], (float)M[10], (float)M[11], (float)(M[0] * fx + M[1] * fy + M[2]));
    *reinterpret_cast<float4*>(o + 4) = make_float4((float)(M[3] * fx + M[4] * fy + M[5]), (float)(M[6] * fx + M[7] * fy + M[8]),
                                                    (float)x, (float)y);
}
void launch_gen_rays_at(const float* tar_ext, const float* tar_ixt, const int* xy, int B, int N, float scale, float* rays,
                        hipStream_t st) {
    ENERF_LAUNCH(k_gen_rays_at, (unsigned)(cdiv(N, 256) * B), 256, 0, st, tar_ext, tar_ixt, xy, B, N, scale, rays);
}

// -------------------------------------------------------------------------------------------------
// gen_rays_bbox (lib/utils/net_utils.py:13-28): slab test of every ray against the axis-aligned box `bounds` (2,3), the
// origin taken from the FIRST ray (rays_o[:1], as the reference does).  Bit-exact restatement: fp32, no fma contraction,
// the reference's direction clamps (|v| pushed away from 0 to +-1e-5) and min/max order.  mask[i] = near < far.
// -------------------------------------------------------------------------------------------------
__device__ __forceinline__ float mul_rn(float a, float b) {
#ifdef ENERF_EMU
    return a * b;
#else
    return __fmul_rn(a, b);
#endif
}
__device__ __forceinline__ float add_rn(float a, float b) {
#ifdef ENERF_EMU
    return a + b;
#else
    return __fadd_rn(a, b);
#endif
}
__global__ __launch_bounds__(256) void k_rays_bbox_mask(const float* __restrict__ rays, const float* __restrict__ bounds,
                                                        long long n, int* __restrict__ mask) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float* r = rays + i * 8;
    const float dx = r[3], dy = r[4], dz = r[5];
    const float nrm = sqrtf(add_rn(add_rn(mul_rn(dx, dx), mul_rn(dy, dy)), mul_rn(dz, dz)));     // torch.norm(dim=-1)
    float v[3] = {dx / nrm, dy / nrm, dz / nrm};
    float near = -INFINITY, far = INFINITY;
    for (int c = 0; c < 3; ++c) {
        if (v[c] < 1e-5f && v[c] > -1e-10f) v[c] = 1e-5f;
        if (v[c] > -1e-5f && v[c] < 1e-10f) v[c] = -1e-5f;
        const float o = rays[c];                                       // rays_o[:1]
        const float t0 = add_rn(bounds[c], -o) / v[c], t1 = add_rn(bounds[3 + c], -o) / v[c];
        near = fmaxf(near, fminf(t0, t1));
        far = fminf(far, fmaxf(t0, t1));
    }
    mask[i] = near < far ? 1 : 0;
}
void launch_rays_bbox_mask(const float* rays, const float* bounds, long long n, int* mask, hipStream_t st) {
    ENERF_LAUNCH_SIMPLE(k_rays_bbox_mask, (unsigned)cdivl(n, 256), 256, 0, st, rays, bounds, n, mask);
}

// -------------------------------------------------------------------------------------------------
// Nearest-view selection of the interactive dataset (zjumocap/enerf_interactive.py:207-210):
//   distances = ||cam_points - c2w[:3,3]||; near_views = argsort(distances)[:k]
// and the gather of the selected source views into the batch (:214-217): inps (V,H,W,3) -> src_inps (k,3,H,W),
// exts (V,4,4) / ixts (V,3,3) -> (k,...).  One block; V <= 1024 cameras, k <= 8.  Ties resolve to the lower index.
// -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_select_views(const float* __restrict__ cam_points, int V,
                                                      const float* __restrict__ c2w, int k, int* __restrict__ idx) {
    __shared__ double dist[1024];
    for (int v = threadIdx.x; v < V; v += blockDim.x) {
        double s = 0;
        for (int c = 0; c < 3; ++c) { const double d = (double)cam_points[v * 3 + c] - (double)c2w[c * 4 + 3]; s += d * d; }
        dist[v] = s;
    }
    __syncthreads();
    if (threadIdx.x == 0)
        for (int j = 0; j < k; ++j) {
            int best = 0;
            for (int v = 1; v < V; ++v) if (dist[v] < dist[best]) best = v;
            idx[j] = best;
            dist[best] = INFINITY;
        }
}
__global__ __launch_bounds__(256) void k_gather_views(const float* __restrict__ inps, const float* __restrict__ exts,
                                                      const float* __restrict__ ixts, const int* __restrict__ idx, int k,
                                                      int H, int W, float* __restrict__ src_inps,
                                                      float* __restrict__ src_exts, float* __restrict__ src_ixts) {
    const long long hw = (long long)H * W;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;        // over k*H*W pixels
    if (i < (long long)k * 16) src_exts[i] = exts[(long long)idx[i / 16] * 16 + i % 16];
    if (i < (long long)k * 9) src_ixts[i] = ixts[(long long)idx[i / 9] * 9 + i % 9];
    if (i >= k * hw) return;
    const int j = (int)(i / hw);
    const long long p = i - j * hw;
    const float* s = inps + ((long long)idx[j] * hw + p) * 3;
    float* d = src_inps + (long long)j * 3 * hw + p;
    d[0] = s[0]; d[hw] = s[1]; d[2 * hw] = s[2];                         // permute(0,3,1,2)
}
void launch_select_views(const float* cam_points, int V, const float* c2w, int k, int* idx, hipStream_t st) {
    ENERF_LAUNCH(k_select_views, 1u, 256, 0, st, cam_points, V, c2w, k, idx);
}
void launch_gather_views(const float* inps, const float* exts, const float* ixts, const int* idx, int k, int H, int W,
                         float* src_inps, float* src_exts, float* src_ixts, hipStream_t st) {
    ENERF_LAUNCH_SIMPLE(k_gather_views, (unsigned)cdivl((long long)k * H * W, 256), 256, 0, st, inps, exts, ixts, idx, k, H, W,
                        src_inps, src_exts, src_ixts);
}

// -------------------------------------------------------------------------------------------------
// The time frame's images as the camera / decoder delivers them (zjumocap/enerf_interactive.py:116-124,135 read_data and :145
// cache_data, for an undistorted image at input_ratio 1): img (V,H,W,3) uint8 + mask (V,H,W) uint8 -> out (V,3,H,W) float32,
//   keep = dilate(mask != 0, box of `dilate`^2 ones, pixels outside the image do not count);  x = u8 / 255;  x[!keep] = 0;  2x - 1
// so a masked-out pixel is -1.  Bit-exact: the division is the correctly rounded one (no reciprocal), 2x is exact and 2x - 1 rounds
// once whether or not it is contracted into an fma.
//
// Memory-bound (4 bytes read, 12 written per pixel).  A 256-thread block takes a tile of 256 x 16 pixels; a lane owns four
// consecutive pixels of a row, a wave one row of the tile, four passes.  Fast path (W % 4 == 0 and aligned pointers): the lane's 12
// image bytes are three dword loads, every plane gets one float4 store.  Otherwise the same lane walks its four pixels bytewise with
// the row's end checked per pixel.  The dilation is separable: the tile of `keep` bytes with its halo (at most 24 x 264) is staged in
// LDS once, a horizontal pass ORs 2r + 1 neighbours per byte, and the vertical pass ORs 2r + 1 DWORDS — four pixels at a time —
// in registers.  24 x 264 + 24 x 256 bytes of LDS per block.
// -------------------------------------------------------------------------------------------------
constexpr int kIngTW = 256, kIngTH = 16, kIngR = 4;                       // tile; widest halo (dilate 9)
constexpr int kIngRows = kIngTH + 2 * kIngR, kIngPitch = kIngTW + 2 * kIngR;

__device__ __forceinline__ float ingest_value(unsigned u, bool keep) {
    float x = (float)u / 255.f;                                           // IEEE division: what `u8.float() / 255` is
    x = keep ? x : 0.f;
    return 2.f * x - 1.f;
}
__global__ __launch_bounds__(256) void k_ingest_views_u8(const unsigned char* __restrict__ img,
                                                         const unsigned char* __restrict__ mask, int r, int H, int W, int fast,
                                                         float* __restrict__ out) {
    __shared__ unsigned s_raw[kIngRows * kIngPitch / 4];                  // keep bytes of the tile + halo
    __shared__ unsigned s_hor[kIngRows * kIngTW / 4];                     // after the horizontal pass (no horizontal halo left)
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int tx0 = blockIdx.x * kIngTW, ty0 = blockIdx.y * kIngTH;
    const long long hw = (long long)H * W;
    const unsigned char* im = img + (long long)blockIdx.z * hw * 3;
    const unsigned char* mk = mask != nullptr ? mask + (long long)blockIdx.z * hw : nullptr;
    float* o = out + (long long)blockIdx.z * hw * 3;
    const bool dil = mk != nullptr && r > 0;                              // block-uniform
    if (dil) {
        unsigned char* raw = reinterpret_cast<unsigned char*>(s_raw);
        unsigned char* hor = reinterpret_cast<unsigned char*>(s_hor);
        const int rows = kIngTH + 2 * r, cols = kIngTW + 2 * r;
        for (int ry = wave; ry < rows; ry += 4) {
            const int y = ty0 - r + ry;
            for (int rx = lane; rx < cols; rx += 64) {
                const int x = tx0 - r + rx;
                unsigned char k = 0;
                if (y >= 0 && y < H && x >= 0 && x < W) k = mk[(long long)y * W + x] != 0 ? 1 : 0;
                raw[ry * kIngPitch + rx] = k;
            }
        }
        __syncthreads();
        for (int e = tid; e < rows * kIngTW; e += 256) {
            const int ry = e / kIngTW, x = e - ry * kIngTW;
            unsigned k = 0;
            for (int t = 0; t <= 2 * r; ++t) k |= raw[ry * kIngPitch + x + t];
            hor[e] = (unsigned char)k;
        }
        __syncthreads();
    }
    const int x = tx0 + lane * 4;
    for (int pass = 0; pass < kIngTH / 4; ++pass) {
        const int ly = pass * 4 + wave, y = ty0 + ly;
        if (y >= H || x >= W) continue;
        const long long p = (long long)y * W + x;
        unsigned keep4 = 0x01010101u;                                     // one byte per pixel, != 0 = keep
        if (dil) {
            keep4 = 0;
            for (int t = 0; t <= 2 * r; ++t) keep4 |= s_hor[(ly + t) * (kIngTW / 4) + lane];
        } else if (mk != nullptr) {
            if (fast) {
                keep4 = *reinterpret_cast<const unsigned*>(mk + p);
            } else {
                keep4 = 0;
                for (int q = 0; q < 4; ++q)
                    if (x + q < W) keep4 |= (unsigned)mk[p + q] << (8 * q);
            }
        }
        if (fast) {                                                       // W % 4 == 0: the four pixels exist, 12 aligned bytes
            const unsigned* s = reinterpret_cast<const unsigned*>(im + p * 3);
            const unsigned w0 = s[0], w1 = s[1], w2 = s[2];
            const bool k0 = (keep4 & 0xffu) != 0, k1 = (keep4 & 0xff00u) != 0, k2 = (keep4 & 0xff0000u) != 0, k3 = (keep4 >> 24) != 0;
            // bytes: r0 g0 b0 r1 | g1 b1 r2 g2 | b2 r3 g3 b3
            const float4 cr = make_float4(ingest_value(w0 & 255u, k0), ingest_value(w0 >> 24, k1),
                                          ingest_value((w1 >> 16) & 255u, k2), ingest_value((w2 >> 8) & 255u, k3));
            const float4 cg = make_float4(ingest_value((w0 >> 8) & 255u, k0), ingest_value(w1 & 255u, k1),
                                          ingest_value(w1 >> 24, k2), ingest_value((w2 >> 16) & 255u, k3));
            const float4 cb = make_float4(ingest_value((w0 >> 16) & 255u, k0), ingest_value((w1 >> 8) & 255u, k1),
                                          ingest_value(w2 & 255u, k2), ingest_value(w2 >> 24, k3));
            *reinterpret_cast<float4*>(o + p) = cr;
            *reinterpret_cast<float4*>(o + hw + p) = cg;
            *reinterpret_cast<float4*>(o + 2 * hw + p) = cb;
        } else {
            for (int q = 0; q < 4; ++q) {
                if (x + q >= W) break;
                const bool k = ((keep4 >> (8 * q)) & 255u) != 0;
                const unsigned char* s = im + (p + q) * 3;
                o[p + q] = ingest_value(s[0], k);
                o[hw + p + q] = ingest_value(s[1], k);
                o[2 * hw + p + q] = ingest_value(s[2], k);
            }
        }
    }
}
void launch_ingest_views_u8(const unsigned char* img, const unsigned char* mask, int dilate, int V, int H, int W, float* out,
                            hipStream_t st) {
    const int fast = W % 4 == 0 && ((size_t)img & 3) == 0 && ((size_t)mask & 3) == 0 && ((size_t)out & 15) == 0;
    ENERF_LAUNCH(k_ingest_views_u8, dim3((unsigned)cdiv(W, kIngTW), (unsigned)cdiv(H, kIngTH), (unsigned)V), 256, 0, st, img, mask,
                 dilate / 2, H, W, fast, out);
}

// -------------------------------------------------------------------------------------------------
// near_far of the interactive dataset's convert_data (zjumocap/enerf_interactive.py:198-201; zjumocap/enerf.py:163 with 0.1):
//   z = vertices @ ext[:3,:3].T + ext[:3,3];  near_far = [max(min z, near_min), max z]
// vertices (B,n,3), tar_ext (B,4,4) -> near_far (B,2), without the two .item() round trips.  One wave per batch element.
// -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_bounds_near_far(const float* __restrict__ vertices, int n, const float* __restrict__ tar_ext,
                                                        float near_min, float* __restrict__ near_far) {
    const int b = blockIdx.x;
    const float* e = tar_ext + b * 16;
    const float r0 = e[8], r1 = e[9], r2 = e[10], t = e[11];
    float lo = INFINITY, hi = -INFINITY;
    for (int i = threadIdx.x; i < n; i += 64) {
        const float* p = vertices + ((long long)b * n + i) * 3;
        const float z = add_rn(add_rn(add_rn(mul_rn(p[0], r0), mul_rn(p[1], r1)), mul_rn(p[2], r2)), t);
        lo = fminf(lo, z);
        hi = fmaxf(hi, z);
    }
    for (int m = 32; m >= 1; m >>= 1) {
        lo = fminf(lo, __shfl_xor(lo, m));
        hi = fmaxf(hi, __shfl_xor(hi, m));
    }
    if (threadIdx.x == 0) {
        near_far[2 * b] = fmaxf(lo, near_min);
        near_far[2 * b + 1] = hi;
    }
}
void launch_bounds_near_far(const float* vertices, int n, const float* tar_ext, int B, float near_min, float* near_far,
                            hipStream_t st) {
    ENERF_LAUNCH(k_bounds_near_far, (unsigned)B, 64, 0, st, vertices, n, tar_ext, near_min, near_far);
}

// -------------------------------------------------------------------------------------------------
// The boxes of the composite network's foreground layers for one target camera (enerf_outdoor/enerf.py:156-164, read_tar), so that a
// captured viewer loop gets its positions without the host.  One block; lane 8 l + c is corner c of layer l in
// base_utils.get_bound_corners' order (x is bit 2 of c, y bit 1, z bit 0; 0 = the min corner's coordinate), the reductions over a
// layer's eight corners are three xor-shuffles.
//   bounds (L,2,3) world min / max corner, tar_ext (1,4,4), tar_ixt (1,3,3), sizes (w, h) per layer (host) ->
//   xy (L,2) float32, near_far rows 0 .. L-1 = (max(min z, near_min), max z), flags (L)
// Per layer: camera-space corners R p + t; pixels K c divided by z; rintf (np.round's half-to-even); the rectangle of the eight
// rounded points clipped to [0, W-1] x [0, H-1]; x = xmin - floor((w - w_ori) / 2), likewise y (enerf.py:163-164).  The final clamp into
// the image is the frame's (prep_job.h resolve_box_position).  flags: bit 1 = the rectangle is wider or taller than (w, h); bit 2 =
// a corner has z <= 0 (xy is then (0, 0)); bit 3 = the rectangle misses the image.
// NOT read_tar's box bit for bit: that is cv2.boundingRect of a cv2.fillPoly raster of the six faces; the rectangle of the rounded
// corners contains it, so the window never loses content the reference's would keep.
// -------------------------------------------------------------------------------------------------
struct LayerBoxSizes { int w[4], h[4]; };
__global__ __launch_bounds__(64) void k_layer_boxes(const float* __restrict__ bounds, const float* __restrict__ tar_ext,
                                                    const float* __restrict__ tar_ixt, int L, int H, int W, LayerBoxSizes sz,
                                                    float near_min, float* __restrict__ xy, float* __restrict__ near_far,
                                                    int* __restrict__ flags) {
    const int lane = threadIdx.x, l = min(lane >> 3, L - 1), c = lane & 7;      // (lanes past 8 L shadow the last layer and write nothing)
    const float* b = bounds + l * 6;
    const float px = b[((c >> 2) & 1) * 3 + 0], py = b[((c >> 1) & 1) * 3 + 1], pz = b[(c & 1) * 3 + 2];
    float cam[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const float* e = tar_ext + r * 4;
        cam[r] = add_rn(add_rn(add_rn(mul_rn(e[0], px), mul_rn(e[1], py)), mul_rn(e[2], pz)), e[3]);
    }
    const float* K = tar_ixt;
    const float u = add_rn(add_rn(mul_rn(K[0], cam[0]), mul_rn(K[1], cam[1])), mul_rn(K[2], cam[2]));
    const float v = add_rn(add_rn(mul_rn(K[3], cam[0]), mul_rn(K[4], cam[1])), mul_rn(K[5], cam[2]));
    const float z = cam[2];
    // rounded pixel, kept as a float clamped far inside int range (a corner behind the camera, an overflow: flagged, never an address)
    const float big = 1.0e9f;
    const float fx = rintf(u / z), fy = rintf(v / z);
    float xlo = fx >= -big && fx <= big ? fx : (fx > big ? big : -big), ylo = fy >= -big && fy <= big ? fy : (fy > big ? big : -big);
    float xhi = xlo, yhi = ylo, zlo = z, zhi = z;
#pragma unroll
    for (int m = 4; m >= 1; m >>= 1) {
        xlo = fminf(xlo, __shfl_xor(xlo, m)); xhi = fmaxf(xhi, __shfl_xor(xhi, m));
        ylo = fminf(ylo, __shfl_xor(ylo, m)); yhi = fmaxf(yhi, __shfl_xor(yhi, m));
        zlo = fminf(zlo, __shfl_xor(zlo, m)); zhi = fmaxf(zhi, __shfl_xor(zhi, m));
    }
    if (c != 0 || lane >= 8 * L) return;
    const int w = lane >> 3 == 0 ? sz.w[0] : (lane >> 3 == 1 ? sz.w[1] : (lane >> 3 == 2 ? sz.w[2] : sz.w[3]));
    const int h = lane >> 3 == 0 ? sz.h[0] : (lane >> 3 == 1 ? sz.h[1] : (lane >> 3 == 2 ? sz.h[2] : sz.h[3]));
    int f = 0;
    const bool behind = !(zlo > 0.f);                              // (NaN counts as behind)
    const int x0 = (int)xlo, x1 = (int)xhi, y0 = (int)ylo, y1 = (int)yhi;
    if (x1 < 0 || x0 > W - 1 || y1 < 0 || y0 > H - 1) f |= 8;
    const int cx0 = min(max(x0, 0), W - 1), cx1 = min(max(x1, 0), W - 1), cy0 = min(max(y0, 0), H - 1), cy1 = min(max(y1, 0), H - 1);
    const int w_ori = cx1 - cx0 + 1, h_ori = cy1 - cy0 + 1;
    if (w_ori > w || h_ori > h) f |= 2;
    float ox = (float)(cx0 - ((w - w_ori) >> 1)), oy = (float)(cy0 - ((h - h_ori) >> 1));       // (>> of a negative: floor, as Python's //)
    if (behind) { f = 4; ox = 0.f; oy = 0.f; }
    xy[2 * l] = ox;
    xy[2 * l + 1] = oy;
    near_far[2 * l] = fmaxf(zlo, near_min);
    near_far[2 * l + 1] = zhi;
    flags[l] = f;
}
void launch_layer_boxes(const float* bounds, const float* tar_ext, const float* tar_ixt, int L, int H, int W, const int* sizes,
                        float near_min, float* xy, float* near_far, int* flags, hipStream_t st) {
    LayerBoxSizes sz = {};
    for (int l = 0; l < L; ++l) { sz.w[l] = sizes[2 * l]; sz.h[l] = sizes[2 * l + 1]; }
    ENERF_LAUNCH(k_layer_boxes, 1u, 64, 0, st, bounds, tar_ext, tar_ixt, L, H, W, sz, near_min, xy, near_far, flags);
}

// -------------------------------------------------------------------------------------------------
// gui_human.py:88-91:  img *= 255; img.to(uint8); flip(0)   — rgb (H*W,3) float -> (H,W,3) uint8
// -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_pack_rgb8(const float* __restrict__ rgb, int H, int W, int flip,
                                                   unsigned char* __restrict__ out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;       // one thread per pixel
    if (i >= (long long)H * W) return;
    const int y = (int)(i / W), x = (int)(i - (long long)y * W);
    const int yo = flip ? H - 1 - y : y;
    const float* s = rgb + i * 3;
    unsigned char* d = out + ((long long)yo * W + x) * 3;
    for (int c = 0; c < 3; ++c) {
        float v = s[c] * 255.f;
        // bit-exact to torch's `img *= 255; img.to(torch.uint8)` on [0,1] inputs (fp32 multiply, truncation).  Outside
        // [0,1] the reference's C cast is undefined; policy here: saturate (negative / NaN -> 0, > 255 -> 255).
        v = v > 0.f ? (v > 255.f ? 255.f : v) : 0.f;
        d[c] = (unsigned char)(int)v;
    }
}
void launch_pack_rgb8(const float* rgb, int H, int W, int flip, unsigned char* out, hipStream_t st) {
    ENERF_LAUNCH_SIMPLE(k_pack_rgb8, (unsigned)cdivl((long long)H * W, 256), 256, 0, st, rgb, H, W, flip, out);
}

// -------------------------------------------------------------------------------------------------
// Evaluator statistics (evaluators/enerf.py:67-71, 88-103), accumulated into 6 doubles:
//   acc[0] = sum of squared rgb errors over masked pixels (3 channels), acc[1] = their count
//   acc[2] = sum |depth - gt| over gt != 0, acc[3] = count, acc[4] = #(<2), acc[5] = #(<10)
// psnr = 10 log10(acc[1] / acc[0]); abs = acc[2]/acc[3]; acc_2 = acc[4]/acc[3]; acc_10 = acc[5]/acc[3].
// The caller zeroes acc (hipMemsetAsync) before the launch.
// -------------------------------------------------------------------------------------------------
__device__ __forceinline__ double wave_sum(double v) {
    for (int m = 32; m >= 1; m >>= 1) {
        float lo = __int_as_float((int)(__double_as_longlong(v) & 0xffffffffll));
        float hi = __int_as_float((int)(__double_as_longlong(v) >> 32));
        lo = __shfl_xor(lo, m);
        hi = __shfl_xor(hi, m);
        v += __longlong_as_double(((long long)__float_as_int(hi) << 32) | (unsigned int)__float_as_int(lo));
    }
    return v;
}
__global__ __launch_bounds__(256) void k_eval_stats(const float* __restrict__ pred_rgb, const float* __restrict__ gt_rgb,
                                                    const unsigned char* __restrict__ mask, int mask_bytes, long long n_rgb,
                                                    int img_w, int img_h, int crop_h, int crop_w,
                                                    const float* __restrict__ pred_depth,
                                                    const float* __restrict__ gt_depth, long long n_depth,
                                                    double* __restrict__ acc) {
    double a[6] = {0, 0, 0, 0, 0, 0};
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n_rgb; i += stride) {
        bool on = true;
        if (mask != nullptr)                                            // masks = msk >= 1 (evaluators/enerf.py:48)
            on = mask_bytes == 4 ? reinterpret_cast<const int*>(mask)[i] >= 1 : mask[i] >= 1;
        if (img_w > 0) {                                                // eval_center: [crop:-crop] on both axes (:50-54)
            const long long p = i % ((long long)img_w * img_h);
            const int y = (int)(p / img_w), x = (int)(p - (long long)y * img_w);
            on = on && y >= crop_h && y < img_h - crop_h && x >= crop_w && x < img_w - crop_w;
        }
        if (on) {
            for (int c = 0; c < 3; ++c) {                               // skimage psnr: float64 mse
                const double d = (double)pred_rgb[i * 3 + c] - (double)gt_rgb[i * 3 + c];
                a[0] += d * d;
            }
            a[1] += 3.0;
        }
    }
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n_depth; i += stride) {
        const float g = gt_depth[i];
        if (g != 0.f) {
            const float e = fabsf(pred_depth[i] - g);                   // np.abs(float32 - float32): float32 (:96-98)
            a[2] += (double)e; a[3] += 1.0; a[4] += e < 2.f ? 1.0 : 0.0; a[5] += e < 10.f ? 1.0 : 0.0;
        }
    }
    for (int k = 0; k < 6; ++k) {
        const double s = wave_sum(a[k]);
        if ((threadIdx.x & 63) == 0 && s != 0.0) atomicAdd(acc + k, s);
    }
}
void launch_eval_stats(const float* pred_rgb, const float* gt_rgb, const void* mask, int mask_bytes, long long n_rgb,
                       int img_w, int img_h, int crop_h, int crop_w, const float* pred_depth, const float* gt_depth,
                       long long n_depth, double* acc, hipStream_t st) {
    long long n = n_rgb > n_depth ? n_rgb : n_depth;
    long long blocks = cdivl(n, 256);
    unsigned grid = (unsigned)(blocks < 1024 ? (blocks > 0 ? blocks : 1) : 1024);
    ENERF_LAUNCH(k_eval_stats, grid, 256, 0, st, pred_rgb, gt_rgb, (const unsigned char*)mask, mask_bytes, n_rgb, img_w, img_h,
                 crop_h, crop_w, pred_depth, gt_depth, n_depth, acc);
}

// -------------------------------------------------------------------------------------------------
// Evaluator SSIM (evaluators/enerf.py:67-69,76 and enerf_human.py:54-56,64-66): what
// skimage.metrics.structural_similarity(gt, pred, multichannel=True) returns for float32 images — per channel, float64,
// 7x7 uniform window, sample covariance (49/48), data_range 2 (C1 = 4e-4, C2 = 3.6e-3), mean over the windows that lie
// wholly inside the image, mean over the channels.  The image is the rectangle (eval_center crop, or the bounding box of
// the selected mask pixels) with gt and pred zeroed where the mask is off; both are applied while staging, nothing is copied.
//
// Channels are interleaved, so a row of the rectangle is a flat run of 3*rw floats in which the window's horizontal
// neighbours sit 3 floats apart: the kernel works on flat columns and never separates the channels (the three channel means
// have the same window count, so their mean is the sum over all flat columns / (3 * windows)).
//
// Tile: 256 flat output columns x 8 output rows per 256-thread block, one flat column per thread.  Staged: (8+6) rows x
// (256+18) floats of both images = 2 * 14 * 274 * 4 B = 30,688 B of LDS -> 5 blocks (20 waves) per CU, so one block's staging
// loads overlap another's arithmetic; 512 blocks at 512x640.  The halo makes a block read 14/8 * 274/256 = 1.87x its share of the
// image, the excess out of L2 (the tile above staged the same rows).  Measured on MI355X against 16-row tiles (48 KB, 3 blocks per
// CU, one block per CU at 512x640): 16.4 vs 20.1 us per call at 512x640, 37.5 vs 39.8 us at 1024x1024 with the box.
// Each thread walks down its column: per staged row the five 7-tap horizontal sums (x, y, xx, yy, xy) in float64 from 14
// conflict-free 4-byte LDS reads (lanes read consecutive floats), kept in a 7-deep register ring (35 doubles); every row from the
// seventh on adds the ring up (the vertical 7 taps) and forms S.  No 8-byte partial sums go through LDS at all.  One partial per
// block; k_ssim_finish adds them in a fixed order.
// -------------------------------------------------------------------------------------------------
constexpr int kSsimTH = 8, kSsimTF = 256;
constexpr int kSsimRows = kSsimTH + 6, kSsimPitch = kSsimTF + 18;

struct SsimRect { int y0, x0, rh, rw; };
// box (rect_mode 2): {min x - W, min y - H, -max x - 1, -max y - 1} of the selected pixels, all 0 = none selected: every entry is
// an atomicMin target that starts from a zero fill
__device__ __forceinline__ SsimRect ssim_rect(int rect_mode, int img_h, int img_w, int crop_h, int crop_w, const int* box) {
    SsimRect R = {0, 0, img_h, img_w};
    if (rect_mode == 1) { R.y0 = crop_h; R.x0 = crop_w; R.rh = img_h - 2 * crop_h; R.rw = img_w - 2 * crop_w; }
    if (rect_mode == 2) {
        const int x0 = box[0] + img_w, y0 = box[1] + img_h, x1 = -box[2] - 1, y1 = -box[3] - 1;
        R.y0 = y0; R.x0 = x0; R.rh = y1 - y0 + 1; R.rw = x1 - x0 + 1;
        if (box[0] == 0) { R.y0 = 0; R.x0 = 0; R.rh = 0; R.rw = 0; }
    }
    return R;
}
// mask_mode 0: value >= 1 (evaluators/enerf.py:48), 1: value == 1 (enerf_human.py:54)
__device__ __forceinline__ bool ssim_mask_on(const unsigned char* mask, int mask_bytes, int mask_mode, long long i) {
    const int v = mask_bytes == 4 ? reinterpret_cast<const int*>(mask)[i] : (int)mask[i];
    return mask_mode ? v == 1 : v >= 1;
}

// cv2.boundingRect(mask) (enerf_human.py:64) on the device: grid (blocks, B), box (B,4) zeroed by the caller.  A block takes whole
// rows (no division per pixel), reduces to four values and sends at most four atomics, none where the box already covers its own
// (a stale read only errs towards sending one: the entries only ever decrease).
__global__ __launch_bounds__(256) void k_mask_bbox(const unsigned char* __restrict__ mask, int mask_bytes, int mask_mode,
                                                   int img_h, int img_w, int* box) {
    __shared__ int wmin[4][4];
    const int b = blockIdx.y, tid = threadIdx.x;
    int m[4] = {0, 0, 0, 0};
    for (int y = blockIdx.x; y < img_h; y += gridDim.x) {
        const long long row = ((long long)b * img_h + y) * img_w;
        for (int x = tid; x < img_w; x += 256)
            if (ssim_mask_on(mask, mask_bytes, mask_mode, row + x)) {
                m[0] = min(m[0], x - img_w); m[1] = min(m[1], y - img_h); m[2] = min(m[2], -x - 1); m[3] = min(m[3], -y - 1);
            }
    }
    for (int k = 0; k < 4; ++k) {
        for (int s = 32; s >= 1; s >>= 1) m[k] = min(m[k], __shfl_xor(m[k], s));
        if ((tid & 63) == 0) wmin[tid >> 6][k] = m[k];
    }
    __syncthreads();
    if (tid < 4) {
        const int v = min(min(wmin[0][tid], wmin[1][tid]), min(wmin[2][tid], wmin[3][tid]));
        if (v != 0 && box[b * 4 + tid] > v) atomicMin(box + b * 4 + tid, v);
    }
}

// S of one window and channel from its five 49-term sums {x, y, xx, yy, xy} (_structural_similarity.py:188-208).  No fma
// contraction: identical images must give A1 == B1 and A2 == B2 bit for bit, hence S == 1.0 exactly.
__device__ __forceinline__ double ssim_window(double sx, double sy, double sxx, double syy, double sxy) {
#ifndef ENERF_EMU
#pragma clang fp contract(off)
#endif
    const double inv = 1.0 / 49.0, cov = 49.0 / 48.0;
    const double C1 = (0.01 * 2.0) * (0.01 * 2.0), C2 = (0.03 * 2.0) * (0.03 * 2.0);
    const double ux = sx * inv, uy = sy * inv, uxx = sxx * inv, uyy = syy * inv, uxy = sxy * inv;
    const double vx = cov * (uxx - ux * ux), vy = cov * (uyy - uy * uy), vxy = cov * (uxy - ux * uy);
    const double A1 = 2.0 * ux * uy + C1, A2 = 2.0 * vxy + C2;
    const double B1 = ux * ux + uy * uy + C1, B2 = vx + vy + C2;
    return (A1 * A2) / (B1 * B2);
}

// grid (flat-column tiles, row tiles, B); partial (B, gridDim.x * gridDim.y): every block writes its own entry (0 when its
// tile lies outside the rectangle, which in rect_mode 2 only the device knows)
__global__ __launch_bounds__(256) void k_ssim_moments(const float* __restrict__ pred, const float* __restrict__ gt,
                                                      const unsigned char* __restrict__ mask, int mask_bytes, int mask_mode,
                                                      int img_h, int img_w, int rect_mode, int crop_h, int crop_w,
                                                      const int* __restrict__ box, double* __restrict__ partial) {
    __shared__ float lx[kSsimRows * kSsimPitch], ly[kSsimRows * kSsimPitch];
    __shared__ double wsum[4];
    const int tid = threadIdx.x, b = blockIdx.z;
    double* out = partial + (long long)b * (gridDim.x * gridDim.y) + (blockIdx.y * gridDim.x + blockIdx.x);
    const SsimRect R = ssim_rect(rect_mode, img_h, img_w, crop_h, crop_w, box + b * 4);
    const int oy0 = blockIdx.y * kSsimTH, of0 = blockIdx.x * kSsimTF;       // first output row / flat column of the tile
    const int out_h = R.rh - 6, out_f = (R.rw - 6) * 3, in_f = R.rw * 3;
    if (oy0 >= out_h || of0 >= out_f) {                                     // block-uniform (also: rectangle under 7x7)
        if (tid == 0) *out = 0.0;
        return;
    }
    const long long img0 = (long long)b * img_h * img_w;
    // a fixed trip count, unrolled, and the three loads of an element independent of each other (the mask selects afterwards): the
    // loads of several elements are in flight together instead of one memory round trip after the other
    constexpr int kStage = (kSsimRows * kSsimPitch + 255) / 256;
#pragma unroll 8
    for (int it = 0; it < kStage; ++it) {
        const int e = it * 256 + tid;
        const int r = e / kSsimPitch, f = e - r * kSsimPitch;
        const int ry = oy0 + r, rf = of0 + f;                               // row / flat column inside the rectangle
        float vx = 0.f, vy = 0.f;
        if (r < kSsimRows && ry < R.rh && rf < in_f) {
            const int px = rf / 3;
            const long long pix = img0 + (long long)(R.y0 + ry) * img_w + (R.x0 + px);
            const bool on = mask == nullptr || ssim_mask_on(mask, mask_bytes, mask_mode, pix);   // gt[mask == False] = 0 (:68-69)
            const float gx = gt[pix * 3 + (rf - px * 3)], gy = pred[pix * 3 + (rf - px * 3)];
            vx = on ? gx : 0.f;
            vy = on ? gy : 0.f;
        }
        if (r < kSsimRows) { lx[e] = vx; ly[e] = vy; }
    }
    __syncthreads();
    const bool col_on = of0 + tid < out_f;
    double h[7][5];
    double acc = 0.0;
#pragma unroll
    for (int r = 0; r < kSsimRows; ++r) {
        const float* px = lx + r * kSsimPitch + tid;
        const float* py = ly + r * kSsimPitch + tid;
        double s[5] = {0, 0, 0, 0, 0};
#pragma unroll
        for (int t = 0; t < 7; ++t) {                                       // products of two fp32 values: exact in fp64
            const double x = (double)px[3 * t], y = (double)py[3 * t];
            s[0] += x; s[1] += y; s[2] += x * x; s[3] += y * y; s[4] += x * y;
        }
#pragma unroll
        for (int k = 0; k < 5; ++k) h[r % 7][k] = s[k];
        if (r >= 6) {
            double m[5];
#pragma unroll
            for (int k = 0; k < 5; ++k) m[k] = ((h[0][k] + h[1][k]) + (h[2][k] + h[3][k])) + ((h[4][k] + h[5][k]) + h[6][k]);
            const double S = ssim_window(m[0], m[1], m[2], m[3], m[4]);
            if (col_on && oy0 + (r - 6) < out_h) acc += S;
        }
    }
    acc = wave_sum(acc);
    if ((tid & 63) == 0) wsum[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) *out = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
}

// one block per image: the partials in a fixed order (strided per thread, butterfly per wave, the four waves in order), then
// out[b] = {mean S, windows per channel}; a rectangle under 7x7 (empty or tiny bounding box): {NaN, 0}
__global__ __launch_bounds__(256) void k_ssim_finish(const double* __restrict__ partial, int nblk, int img_h, int img_w,
                                                     int rect_mode, int crop_h, int crop_w, const int* __restrict__ box,
                                                     double* __restrict__ out) {
    __shared__ double wsum[4];
    const int tid = threadIdx.x, b = blockIdx.x;
    double a = 0.0;
    for (int i = tid; i < nblk; i += 256) a += partial[(long long)b * nblk + i];
    a = wave_sum(a);
    if ((tid & 63) == 0) wsum[tid >> 6] = a;
    __syncthreads();
    if (tid != 0) return;
    const SsimRect R = ssim_rect(rect_mode, img_h, img_w, crop_h, crop_w, box + b * 4);
    const bool ok = R.rh >= 7 && R.rw >= 7;
    const double n = ok ? (double)(R.rh - 6) * (double)(R.rw - 6) : 0.0;
    out[2 * b] = ok ? ((wsum[0] + wsum[1]) + (wsum[2] + wsum[3])) / (3.0 * n) : NAN;
    out[2 * b + 1] = n;
}

static void ssim_grid(int img_h, int img_w, int rect_mode, int crop_h, int crop_w, int* tiles_f, int* tiles_y) {
    const int rh = rect_mode == 1 ? img_h - 2 * crop_h : img_h, rw = rect_mode == 1 ? img_w - 2 * crop_w : img_w;
    *tiles_f = cdiv((rw - 6) * 3, kSsimTF);
    *tiles_y = cdiv(rh - 6, kSsimTH);
}
size_t eval_ssim_workspace_bytes(int B, int img_h, int img_w, int rect_mode, int crop_h, int crop_w) {
    int tf, ty;
    ssim_grid(img_h, img_w, rect_mode, crop_h, crop_w, &tf, &ty);
    return (size_t)B * 16 + (size_t)B * tf * ty * sizeof(double);          // boxes (B,4) int32 | partials (B, tiles) double
}
void launch_eval_ssim(const float* pred_rgb, const float* gt_rgb, const void* mask, int mask_bytes, int mask_mode, int B,
                      int img_h, int img_w, int rect_mode, int crop_h, int crop_w, void* workspace, double* out,
                      hipStream_t st) {
    int tf, ty;
    ssim_grid(img_h, img_w, rect_mode, crop_h, crop_w, &tf, &ty);
    int* box = (int*)workspace;
    double* partial = (double*)((char*)workspace + (size_t)B * 16);
    if (rect_mode == 2) {
        zero_async(box, (size_t)B * 16, st);
        ENERF_LAUNCH(k_mask_bbox, dim3((unsigned)(img_h < 512 ? img_h : 512), (unsigned)B), 256, 0, st, (const unsigned char*)mask,
                     mask_bytes, mask_mode, img_h, img_w, box);
    }
    ENERF_LAUNCH(k_ssim_moments, dim3((unsigned)tf, (unsigned)ty, (unsigned)B), 256, 0, st, pred_rgb, gt_rgb,
                 (const unsigned char*)mask, mask_bytes, mask_mode, img_h, img_w, rect_mode, crop_h, crop_w, box, partial);
    ENERF_LAUNCH(k_ssim_finish, (unsigned)B, 256, 0, st, partial, tf * ty, img_h, img_w, rect_mode, crop_h, crop_w, box, out);
}

}  // namespace enerf

// Evaluator LPIPS (evaluators/enerf.py:81-87, enerf_human.py:71-77): the VGG16 trunk and the taps
#include "lpips_vgg.h"
// Trainer's perceptual term (losses/vgg_perceptual_loss.py:21-37): the same trunk's first ten layers, forward and backward
#include "perceptual_vgg.h"
// Raw camera frames (undistort, area resize, crop) to the float image of the source-view caches (enerf_outdoor/enerf.py:129-152)
#include "ingest_raw.h"
// The foreground's world-space box of a time frame, carved from the masks (the reference loads it from vhull/*.npy made offline)
#include "vhull.h"
