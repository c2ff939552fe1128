// ingest_raw.h — raw camera frames to the float image the source-view caches are built from, on the device (included by io.hip).
//
// What the reference's datasets do on the host per view and per time frame (zjumocap/enerf_interactive.py:116-135, zjumocap/enerf.py:
// 141-149, enerf_outdoor/enerf.py:129-152): cv2.undistort of image and mask, an INTER_AREA / INTER_NEAREST resize by input_ratio, the
// mask dilated in front and zeroed behind, a crop with the intrinsics moved along.  Here:
//   img (V,Hraw,Wraw,3) uint8 [+ mask (V,Hraw,Wraw)], K (V,3,3), D (V,5) = (k1,k2,p1,p2,k3) or none  ->  out (V,3,H,W) float32 in [-1,1]
//   x = u8 / 255 (correctly rounded);  keep_raw = dilate(mask != 0)
//   undistort: pixel (u,v) of the undistorted image (same size, same K) samples the raw image at
//       a = (u-cx)/fx, b = (v-cy)/fy, r2 = a^2+b^2, rad = 1 + r2 (k1 + r2 (k2 + r2 k3))
//       u' = fx (a rad + 2 p1 a b + p2 (r2 + 2 a^2)) + cx,   v' = fy (b rad + p1 (r2 + 2 b^2) + 2 p2 a b) + cy
//     bilinearly, taps outside the raw image contribute 0; the undistorted mask is kept where the weight of its kept taps is >= 0.5
//   resize: Hs x Ws = Hraw r, Wraw r rounded half-to-even, s = 1/r; output pixel d of an axis averages the undistorted pixels j with
//     weight |[d s, (d+1) s) n [j, j+1) n [0, src)| normalised to 1, separably (INTER_AREA); the mask takes j = min(floor(d s), src-1)
//   crop (y0, x0, H, W) of the resized image, x[!keep] = 0, 2x - 1
// Every coordinate and weight is double (a float32 map costs 1e-4 px at 1024^2); pixel values and their sums are float32.  Without D
// the bilinear step does not exist (not: runs with zero coefficients), and at r = 1 without a crop every weight is exactly 1, so the
// result is k_ingest_views_u8's bit for bit.
// NOT cv2's bits: no 1/32-pixel rounding of the map, no dropped overlaps under 1e-3 px, another summation order.
//
// One 256-thread block per 32 x 8 output tile.  Prologue: wave 0 computes the <= 6 area taps of the tile's 32 columns, wave 1 those of
// its 8 rows.  Then the block evaluates the undistorted float RGB footprint of its tile ONCE into LDS, planar: (ceil(8 s) + 2) rows of
// (ceil(32 s) + 2) floats per channel, 53,040 bytes at r = 0.25 and 4,080 at r = 1 (dynamic, so the occupancy follows r).  A footprint
// pixel is one double map evaluation and four raw taps of three bytes: the map's two divisions, (u - cx) / fx and (v - cy) / fy, are
// done once per footprint column and row (two small LDS tables), the two taps of a raw row are ONE 8-byte load of any alignment
// where both exist (bytewise from clamped positions at the image's rim), and u8 / 255 is a Newton step on the rounded reciprocal,
// the correctly rounded quotient at all 256 values, instead of twelve expanded divisions.  The mask needs only the ONE undistorted
// pixel under each output pixel: thread t does output pixel t's map and its four taps of the (dilated) raw mask.  Last, three waves
// (one per channel) reduce the area weights out of LDS, four pixels of a row per lane, taps and weights in registers, and store one
// float4 per lane where W % 4 == 0.
// No input can form an address outside the raw image: (u', v') is tested in double against (-1, W) x (-1, H) BEFORE any conversion to
// an integer (NaN, inf, fx = 0 and wild coefficients fail the test and give 0), and the tap indices are clamped after it.
// The dilation of a raw mask runs in front as a launch of its own (k_dilate_mask_u8, the separable LDS dilation of k_ingest_views_u8
// writing bytes instead of consuming them) into the caller's scratch (V,Hraw,Wraw).

namespace enerf {

constexpr int kRawTW = 32, kRawTH = 8, kRawTaps = 6;          // output tile; most area taps per axis (s <= 4: 4 whole + 2 partial)

struct RawAxis { int j0, n; float w[kRawTaps]; };             // taps j0 .. j0+n-1 of one output column / row
struct RawGeom {
    int Hraw, Wraw, H, W, crop_y, crop_x;
    int fpitch, frows;                                        // the footprint's LDS extents
    double s;                                                 // 1 / input_ratio
};

__host__ __device__ __forceinline__ int raw_foot_extent(int tile, double s) { return (int)ceil((double)tile * s) + 2; }

// area taps of output pixel d on an axis of `src` undistorted pixels
__device__ __forceinline__ void raw_area_axis(int d, double s, int src, RawAxis* A) {
    const double fs = (double)src;
    double lo = (double)d * s, hi = ((double)d + 1.0) * s;
    lo = lo < fs ? lo : fs;
    hi = hi < fs ? hi : fs;
    const int a = (int)floor(lo), b = (int)ceil(hi);
    int n = b - a;
    n = n < kRawTaps ? n : kRawTaps;                          // (never more: see kRawTaps)
    double ov[kRawTaps], tot = 0.0;
    for (int t = 0; t < kRawTaps; ++t) {
        const double j = (double)(a + t);
        const double o = (hi < j + 1.0 ? hi : j + 1.0) - (lo > j ? lo : j);
        ov[t] = t < n && o > 0.0 ? o : 0.0;
        tot += ov[t];
    }
    A->j0 = a;
    A->n = n > 0 ? n : 0;
    const double inv = tot > 0.0 ? 1.0 / tot : 0.0;
    for (int t = 0; t < kRawTaps; ++t) A->w[t] = (float)(ov[t] * inv);
}

// the raw-image position the undistorted pixel (u, v) samples: false = no tap lies inside the raw image (or the map is not finite);
// else x0, y0 in [-1, W-1] x [-1, H-1] and the fractions
struct RawCam { double fx, fy, cx, cy, k1, k2, p1, p2, k3; };
__device__ __forceinline__ RawCam raw_cam(const float* __restrict__ K, const float* __restrict__ D) {
    RawCam c;
    c.fx = (double)K[0]; c.cx = (double)K[2]; c.fy = (double)K[4]; c.cy = (double)K[5];
    c.k1 = (double)D[0]; c.k2 = (double)D[1]; c.p1 = (double)D[2]; c.p2 = (double)D[3]; c.k3 = (double)D[4];
    return c;
}
// a = (u - cx) / fx depends on the column alone and b = (v - cy) / fy on the row: the block divides once per footprint column and row
__device__ __forceinline__ bool raw_map(const RawCam& c, double a, double b, int Hraw, int Wraw, int* x0, int* y0, double* ax, double* ay) {
    const double r2 = a * a + b * b;
    const double rad = 1.0 + r2 * (c.k1 + r2 * (c.k2 + r2 * c.k3));
    const double a2 = a * rad + 2.0 * c.p1 * a * b + c.p2 * (r2 + 2.0 * a * a);
    const double b2 = b * rad + c.p1 * (r2 + 2.0 * b * b) + 2.0 * c.p2 * a * b;
    const double us = c.fx * a2 + c.cx, vs = c.fy * b2 + c.cy;
    if (!(us > -1.0 && us < (double)Wraw && vs > -1.0 && vs < (double)Hraw)) return false;      // NaN fails; tested before any int
    const double fu = floor(us), fv = floor(vs);
    *ax = us - fu;
    *ay = vs - fv;
    *x0 = min(max((int)fu, -1), Wraw - 1);
    *y0 = min(max((int)fv, -1), Hraw - 1);
    return true;
}

// (float)b / 255.f for b in 0 .. 255 without the division's expansion: one Newton step on the rounded reciprocal, which is the
// correctly rounded quotient at every one of the 256 values (checked exhaustively on the host; tests: all 256 values through the
// bilinear path at weight 1 equal the division's bits)
__device__ __forceinline__ float raw_unit(unsigned b) {
    const float r = 1.f / 255.f, fb = (float)b;
    const float q = fb * r;
    return fmaf(fmaf(-q, 255.f, fb), r, q);
}
// the two taps x0, x0 + 1 of one raw row: r0 g0 b0 r1 g1 b1 in the low six bytes.  `wide`: both taps exist and eight bytes from the
// first lie inside the view — one load of any alignment; else bytewise from clamped positions (a tap outside has weight 0)
__device__ __forceinline__ unsigned long long raw_row_taps(const unsigned char* __restrict__ row, int x0, int Wraw, bool wide) {
    unsigned long long t = 0;
    if (wide) {
        __builtin_memcpy(&t, row + x0 * 3, 8);
    } else {
        const unsigned char* p0 = row + min(max(x0, 0), Wraw - 1) * 3;
        const unsigned char* p1 = row + min(max(x0 + 1, 0), Wraw - 1) * 3;
        t = (unsigned long long)p0[0] | ((unsigned long long)p0[1] << 8) | ((unsigned long long)p0[2] << 16) |
            ((unsigned long long)p1[0] << 24) | ((unsigned long long)p1[1] << 32) | ((unsigned long long)p1[2] << 40);
    }
    return t;
}

constexpr int kRawFootW = 4 * kRawTW + 2, kRawFootH = 4 * kRawTH + 2;     // the footprint's largest extents (s = 4)

template <bool DIST, bool MASK>
__global__ __launch_bounds__(256) void k_ingest_raw_u8(const unsigned char* __restrict__ img, const unsigned char* __restrict__ mask,
                                                       const float* __restrict__ ixts, const float* __restrict__ dist, RawGeom g,
                                                       int fast, float* __restrict__ out, unsigned char* __restrict__ mask_out) {
    ENERF_DYN_SMEM(float, foot);                                          // [3][frows][fpitch]
    __shared__ RawAxis s_ax[kRawTW], s_ay[kRawTH];
    __shared__ unsigned char s_keep[kRawTW * kRawTH];
    __shared__ double s_a[DIST ? kRawFootW : 1], s_b[DIST ? kRawFootH : 1];   // (u - cx) / fx per footprint column, (v - cy) / fy per row
    const int tid = threadIdx.x, view = blockIdx.z;
    const int X0 = blockIdx.x * kRawTW, Y0 = blockIdx.y * kRawTH;         // the tile in the output image
    const int Hraw = g.Hraw, Wraw = g.Wraw;
    const long long hw_raw = (long long)Hraw * Wraw;
    const unsigned char* im = img + (long long)view * hw_raw * 3;
    const int tw = min(kRawTW, g.W - X0), th = min(kRawTH, g.H - Y0);     // the tile's valid extent (>= 1 by the grid)

    if (tid < tw) raw_area_axis(g.crop_x + X0 + tid, g.s, Wraw, &s_ax[tid]);                    // wave 0: the columns
    else if (tid >= 64 && tid - 64 < th) raw_area_axis(g.crop_y + Y0 + tid - 64, g.s, Hraw, &s_ay[tid - 64]);   // wave 1: the rows
    __syncthreads();
    // the footprint: undistorted pixels [fx0, fx0 + fw) x [fy0, fy0 + fh), inside the image by construction (taps end at src)
    const int fx0 = s_ax[0].j0, fy0 = s_ay[0].j0;
    const int fw = min(s_ax[tw - 1].j0 + s_ax[tw - 1].n - fx0, g.fpitch), fh = min(s_ay[th - 1].j0 + s_ay[th - 1].n - fy0, g.frows);
    const int plane = g.frows * g.fpitch;
    const unsigned view_bytes = (unsigned)(hw_raw * 3);
    RawCam cam = {};
    if (DIST) {
        cam = raw_cam(ixts + view * 9, dist + view * 5);
        if (tid < fw) s_a[tid] = ((double)min(fx0 + tid, Wraw - 1) - cam.cx) / cam.fx;
        else if (tid >= 192 && tid - 192 < fh) s_b[tid - 192] = ((double)min(fy0 + tid - 192, Hraw - 1) - cam.cy) / cam.fy;
        __syncthreads();
    }
    for (int e = tid; e < fw * fh; e += 256) {
        const int fy = e / fw, fx = e - fy * fw;
        const int u = min(fx0 + fx, Wraw - 1), v = min(fy0 + fy, Hraw - 1);
        float c0 = 0.f, c1 = 0.f, c2 = 0.f;
        if (DIST) {
            int x0, y0;
            double ax, ay;
            if (raw_map(cam, s_a[fx], s_b[fy], Hraw, Wraw, &x0, &y0, &ax, &ay)) {
                const bool xin0 = x0 >= 0, xin1 = x0 + 1 < Wraw;
#pragma unroll
                for (int ty = 0; ty < 2; ++ty) {
                    const int y = y0 + ty;
                    const bool yin = y >= 0 && y < Hraw;
                    const unsigned ro = (unsigned)min(max(y, 0), Hraw - 1) * (unsigned)(Wraw * 3);     // (a view is under 2^32 bytes)
                    const bool wide = xin0 && xin1 && ro + (unsigned)(x0 * 3) + 8u <= view_bytes;
                    const unsigned long long t = raw_row_taps(im + ro, x0, Wraw, wide);
                    const unsigned lo = (unsigned)t, hi = (unsigned)(t >> 32);
                    const double wy = ty ? ay : 1.0 - ay;
                    const float w0 = yin && xin0 ? (float)((1.0 - ax) * wy) : 0.f, w1 = yin && xin1 ? (float)(ax * wy) : 0.f;
                    c0 += w0 * raw_unit(lo & 255u);
                    c1 += w0 * raw_unit((lo >> 8) & 255u);
                    c2 += w0 * raw_unit((lo >> 16) & 255u);
                    c0 += w1 * raw_unit(lo >> 24);
                    c1 += w1 * raw_unit(hi & 255u);
                    c2 += w1 * raw_unit((hi >> 8) & 255u);
                }
            }
        } else {
            const unsigned char* p = im + ((long long)v * Wraw + u) * 3;
            c0 = (float)p[0] / 255.f;
            c1 = (float)p[1] / 255.f;
            c2 = (float)p[2] / 255.f;
        }
        float* f = foot + fy * g.fpitch + fx;
        f[0] = c0; f[plane] = c1; f[2 * plane] = c2;
    }
    if (MASK) {                                                           // output pixel tid: the one undistorted mask pixel under it
        const int ly = tid / kRawTW, lx = tid - ly * kRawTW;
        if (ly < th && lx < tw) {
            const unsigned char* mk = mask + (long long)view * hw_raw;
            const int ju = min((int)floor((double)(g.crop_x + X0 + lx) * g.s), Wraw - 1);
            const int jv = min((int)floor((double)(g.crop_y + Y0 + ly) * g.s), Hraw - 1);
            bool keep = false;
            if (DIST) {
                int x0, y0;
                double ax, ay;
                // (ju, jv) is the first area tap of its column / row, so it lies in the footprint and its a, b are in the tables
                if (raw_map(cam, s_a[min(max(ju - fx0, 0), kRawFootW - 1)], s_b[min(max(jv - fy0, 0), kRawFootH - 1)], Hraw, Wraw, &x0, &y0,
                            &ax, &ay)) {
                    double kept = 0.0;
#pragma unroll
                    for (int t = 0; t < 4; ++t) {
                        const int x = x0 + (t & 1), y = y0 + (t >> 1);
                        const bool in = x >= 0 && x < Wraw && y >= 0 && y < Hraw;
                        const unsigned char m = mk[(long long)min(max(y, 0), Hraw - 1) * Wraw + min(max(x, 0), Wraw - 1)];
                        if (in && m != 0) kept += ((t & 1) ? ax : 1.0 - ax) * ((t >> 1) ? ay : 1.0 - ay);
                    }
                    keep = kept >= 0.5;
                }
            } else {
                keep = mk[(long long)jv * Wraw + ju] != 0;
            }
            s_keep[tid] = keep ? 1 : 0;
            if (mask_out != nullptr) mask_out[((long long)view * g.H + Y0 + ly) * g.W + X0 + lx] = keep ? 1 : 0;
        }
    }
    __syncthreads();
    // three waves, one per channel: lane = (row of the tile, four pixels of it)
    const int c = tid >> 6, lane = tid & 63, ly = lane >> 3, lx4 = (lane & 7) * 4;
    if (c >= 3 || ly >= th || lx4 >= tw) return;
    const RawAxis ay = s_ay[ly];                                          // in registers: the loops below are unrolled over kRawTaps
    const float* fc = foot + c * plane;
    const int ry0 = ay.j0 - fy0;
    float r4[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        if (lx4 + q >= tw) break;
        const RawAxis ax = s_ax[lx4 + q];
        const int rx0 = ax.j0 - fx0;
        float acc = 0.f;
#pragma unroll
        for (int ty = 0; ty < kRawTaps; ++ty) {                           // (the clamps never bind: the footprint ends at the last tap)
            if (ty >= ay.n) continue;
            const float* f = fc + min(ry0 + ty, g.frows - 1) * g.fpitch;
            float row = 0.f;
#pragma unroll
            for (int tx = 0; tx < kRawTaps; ++tx)
                if (tx < ax.n) row += ax.w[tx] * f[min(rx0 + tx, g.fpitch - 1)];
            acc += ay.w[ty] * row;
        }
        const bool keep = !MASK || s_keep[ly * kRawTW + lx4 + q] != 0;
        acc = keep ? acc : 0.f;
        r4[q] = 2.f * acc - 1.f;
    }
    const long long hw = (long long)g.H * g.W;
    float* o = out + ((long long)view * 3 + c) * hw + (long long)(Y0 + ly) * g.W + X0 + lx4;
    if (fast) {                                                           // W % 4 == 0: the four pixels exist, 16 aligned bytes
        *reinterpret_cast<float4*>(o) = make_float4(r4[0], r4[1], r4[2], r4[3]);
    } else {
        for (int q = 0; q < 4 && lx4 + q < tw; ++q) o[q] = r4[q];
    }
}

// keep = dilate(mask != 0) as bytes 0 / 1: k_ingest_views_u8's box and border rule (pixels outside the image do not count) and its
// tile; the vertical pass's dword of four pixels is stored instead of consumed.  With W % 4 == 0 and aligned pointers the tile is
// staged as DWORDS — 66 per row, one of halo on either side (r <= 4), at most seven independent loads per thread in flight together
// instead of the bytewise staging's 25 dependent round trips — and the horizontal pass ORs the 2r + 1 byte shifts of a 12-byte window.
constexpr int kDilPitchW = kIngTW / 4 + 2;
__device__ __forceinline__ unsigned raw_nonzero_bytes(unsigned v) {       // byte i = (byte i of v != 0)
    return ((v | ((v & 0x7f7f7f7fu) + 0x7f7f7f7fu)) >> 7) & 0x01010101u;
}
__global__ __launch_bounds__(256) void k_dilate_mask_u8(const unsigned char* __restrict__ mask, int r, int H, int W, int fast,
                                                        unsigned char* __restrict__ keep) {
    __shared__ unsigned s_raw[kIngRows * kDilPitchW];                     // (== kIngRows * kIngPitch bytes: the bytewise path's tile)
    __shared__ unsigned s_hor[kIngRows * kIngTW / 4];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int tx0 = blockIdx.x * kIngTW, ty0 = blockIdx.y * kIngTH;
    const long long hw = (long long)H * W;
    const unsigned char* mk = mask + (long long)blockIdx.z * hw;
    unsigned char* o = keep + (long long)blockIdx.z * hw;
    const int rows = kIngTH + 2 * r, cols = kIngTW + 2 * r;
    if (fast) {
        const int wq = W >> 2, xq0 = (tx0 >> 2) - 1;
        const unsigned* mk4 = reinterpret_cast<const unsigned*>(mk);
#pragma unroll
        for (int it = 0; it < (kIngRows * kDilPitchW + 255) / 256; ++it) {
            const int e = it * 256 + tid;
            const int ry = e / kDilPitchW, dx = e - ry * kDilPitchW;
            const int y = ty0 - r + ry, xq = xq0 + dx;
            unsigned v = 0;
            if (ry < rows && y >= 0 && y < H && xq >= 0 && xq < wq) v = mk4[(long long)y * wq + xq];
            if (ry < rows) s_raw[e] = raw_nonzero_bytes(v);
        }
        __syncthreads();
        for (int e = tid; e < rows * (kIngTW / 4); e += 256) {
            const int ry = e / (kIngTW / 4), xq = e - ry * (kIngTW / 4);
            const unsigned* p = s_raw + ry * kDilPitchW + xq;             // the dwords left of, at and right of the four pixels
            const unsigned long long lc = ((unsigned long long)p[1] << 32) | p[0], cr = ((unsigned long long)p[2] << 32) | p[1];
            unsigned k = p[1];
            for (int t = 1; t <= r; ++t) k |= (unsigned)(lc >> (32 - 8 * t)) | (unsigned)(cr >> (8 * t));
            s_hor[e] = k;
        }
    } else {
        unsigned char* raw = reinterpret_cast<unsigned char*>(s_raw);
        unsigned char* hor = reinterpret_cast<unsigned char*>(s_hor);
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
    }
    __syncthreads();
    const int x = tx0 + lane * 4;
    for (int pass = 0; pass < kIngTH / 4; ++pass) {
        const int ly = pass * 4 + wave, y = ty0 + ly;
        if (y >= H || x >= W) continue;
        unsigned keep4 = 0;
        for (int t = 0; t <= 2 * r; ++t) keep4 |= s_hor[(ly + t) * (kIngTW / 4) + lane];
        const long long p = (long long)y * W + x;
        if (fast) {
            *reinterpret_cast<unsigned*>(o + p) = keep4;
        } else {
            for (int q = 0; q < 4 && x + q < W; ++q) o[p + q] = (unsigned char)((keep4 >> (8 * q)) & 1u);
        }
    }
}

// Hs x Ws of the resized image: Hraw r and Wraw r rounded half-to-even (Python's round, the rule the oracle's resize states)
void ingest_raw_geometry(int Hraw, int Wraw, double r, int* Hs, int* Ws) {
    *Hs = (int)nearbyint((double)Hraw * r);
    *Ws = (int)nearbyint((double)Wraw * r);
}

void launch_ingest_raw_u8(const unsigned char* img, const unsigned char* mask, const float* ixts, const float* dist, int V, int Hraw,
                          int Wraw, double input_ratio, int crop_y, int crop_x, int H, int W, int dilate, unsigned char* mask_scratch,
                          float* out, unsigned char* mask_out, hipStream_t st) {
    if (mask != nullptr && dilate > 0) {
        const int mfast = Wraw % 4 == 0 && ((size_t)mask & 3) == 0 && ((size_t)mask_scratch & 3) == 0;
        ENERF_LAUNCH(k_dilate_mask_u8, dim3((unsigned)cdiv(Wraw, kIngTW), (unsigned)cdiv(Hraw, kIngTH), (unsigned)V), 256, 0, st, mask,
                     dilate / 2, Hraw, Wraw, mfast, mask_scratch);
        mask = mask_scratch;
    }
    RawGeom g;
    g.Hraw = Hraw; g.Wraw = Wraw; g.H = H; g.W = W; g.crop_y = crop_y; g.crop_x = crop_x;
    g.s = 1.0 / input_ratio;
    g.fpitch = raw_foot_extent(kRawTW, g.s);
    g.frows = raw_foot_extent(kRawTH, g.s);
    const size_t lds = (size_t)3 * g.frows * g.fpitch * sizeof(float);    // <= 3 * 34 * 130 * 4 = 53,040 bytes (s <= 4)
    const int fast = W % 4 == 0 && ((size_t)out & 15) == 0;
    const dim3 grid((unsigned)cdiv(W, kRawTW), (unsigned)cdiv(H, kRawTH), (unsigned)V);
    if (dist != nullptr) {
        if (mask != nullptr) ENERF_LAUNCH((k_ingest_raw_u8<true, true>), grid, 256, lds, st, img, mask, ixts, dist, g, fast, out, mask_out);
        else ENERF_LAUNCH((k_ingest_raw_u8<true, false>), grid, 256, lds, st, img, mask, ixts, dist, g, fast, out, mask_out);
    } else {
        if (mask != nullptr) ENERF_LAUNCH((k_ingest_raw_u8<false, true>), grid, 256, lds, st, img, mask, ixts, dist, g, fast, out, mask_out);
        else ENERF_LAUNCH((k_ingest_raw_u8<false, false>), grid, 256, lds, st, img, mask, ixts, dist, g, fast, out, mask_out);
    }
}

}  // namespace enerf
