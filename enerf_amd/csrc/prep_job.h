// prep_job.h — the frame's camera-only preparation (get_proj_mats of every cascade level, utils.py:35-55, and level 0's
// get_depth_values, utils.py:98-111,148-150) as device code that can ride in ANOTHER kernel's launch.
//
// Level 0's depth hypotheses and all projection matrices depend on the batch's cameras and near_far only — not on a single
// feature — yet k_depth_values sat as a 5.8 us launch on the frame's critical chain between the FeatureNet trunk and the warp.
// enerf_forward now appends the job's blocks to the FIRST kernel of the frame (k_conv0_fused_cb): they run beside the
// convolution's blocks, and the launch (and with it the cross-stream bubble in front of it) leaves the chain.  The arithmetic
// is the same device code the stand-alone kernels (geometry.hip) call: identical bits either way.
#pragma once
#include "common.h"

namespace enerf {

// proj3x4 = K'(3x3, rows 0,1 scaled) * E[:3] (3x4)
__device__ __forceinline__ void k_times_e(const float* K, const float* E, float scale, double* out34) {
    for (int r = 0; r < 3; ++r) {
        double sc = r < 2 ? (double)scale : 1.0;
        for (int c = 0; c < 4; ++c) {
            double a = 0;
            for (int k = 0; k < 3; ++k) a += ((double)K[r * 3 + k] * sc) * (double)E[k * 4 + c];
            out34[r * 4 + c] = a;
        }
    }
}
// one (b, s) projection matrix (get_proj_mats utils.py:35-55), fp64 like torch.inverse's LU on these sizes
__device__ __forceinline__ void proj_one(int i, const float* __restrict__ src_ixts, const float* __restrict__ src_exts,
                                         const float* __restrict__ tar_ixt, const float* __restrict__ tar_ext, int S,
                                         float src_scale, float tar_scale, float* __restrict__ proj) {
    const int b = i / S;
    double t44[16], tinv[16], s34[12];
    k_times_e(tar_ixt + b * 9, tar_ext + b * 16, tar_scale, t44);
    t44[12] = t44[13] = t44[14] = 0.0;
    t44[15] = 1.0;
    if (!inv4x4(t44, tinv)) {
        for (int k = 0; k < 16; ++k) tinv[k] = NAN;
    }
    k_times_e(src_ixts + i * 9, src_exts + i * 16, src_scale, s34);
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 4; ++c) {
            double a = 0;
            for (int k = 0; k < 4; ++k) a += s34[r * 4 + k] * tinv[k * 4 + c];
            proj[i * 12 + r * 4 + c] = (float)a;
        }
}

// Optional piggy-backed get_proj_mats of the same level (enerf_level_prep): the B*S fp64 inverses are a 4.7 us
// latency chain in a launch of their own; here the last block's first threads run them next to the plane writes.
struct ProjJob {
    const float *src_ixts, *src_exts, *tar_ixt, *tar_ext;
    float* proj;          // nullptr: no projection matrices in this launch
    int S;
    float src_scale, tar_scale;
};

// one element of get_depth_values' output (B, D, h, w) from the pixel's [nn, ff] (utils.py:104-111 level 0; 137-146 level > 0) and
// the level's near/far planes (utils.py:148-150)
__device__ __forceinline__ void depth_plane_value(float nn, float ff, int b, int k, int p, int D, int hw, int depth_inv,
                                                  float* __restrict__ dv_elem, float* __restrict__ nf_out) {
    const float inn = 1.f / nn, iff = 1.f / ff;
    const float t = linspace01(k, D);
    const float v = depth_inv ? 1.f / (inn + t * (iff - inn)) : nn + t * (ff - nn);
    *dv_elem = v;
    if (k == 0 || k == D - 1) {                  // utils.py:149-150 (k == 0 == D-1 writes both)
        const float e = depth_inv ? 1.f / clamp_min(v, 1e-6f) : v;
        if (k == 0) nf_out[((long long)b * 2 + 0) * hw + p] = e;
        if (k == D - 1) nf_out[((long long)b * 2 + 1) * hw + p] = e;
    }
}

struct PrepJob {
    const float* near_far;     // (B, 2); nullptr: no level-0 planes in this job
    float *dv, *nf;            // level 0: (B, D, h, w), (B, 2, h, w)
    int B, D, h, w, depth_inv;
    ProjJob pj[3];             // projection matrices of up to three cascade levels (proj == nullptr: none)
    int nblocks;               // blocks the job needs at `threads` threads each (dispatched in front of the carrying kernel's own)
};
inline int prep_job_blocks(int B, int D, int h, int w, int threads) { return (B * D * h * w + threads - 1) / threads; }
// block `vb` of the job (threads = blockDim.x of the carrying kernel)
__device__ __forceinline__ void prep_job_block(const PrepJob& J, int vb, int tid, int threads) {
    if (vb == 0) {
#pragma unroll 1
        for (int l = 0; l < 3; ++l)
            if (J.pj[l].proj != nullptr)
                for (int q = tid; q < J.B * J.pj[l].S; q += threads)
                    proj_one(q, J.pj[l].src_ixts, J.pj[l].src_exts, J.pj[l].tar_ixt, J.pj[l].tar_ext, J.pj[l].S, J.pj[l].src_scale,
                             J.pj[l].tar_scale, J.pj[l].proj);
    }
    if (J.near_far == nullptr) return;
    const int i = vb * threads + tid, hw = J.h * J.w;
    if (i >= J.B * J.D * hw) return;
    const int b = i / (J.D * hw), r = i - b * (J.D * hw);
    const int k = r / hw, p = r - k * hw;
    depth_plane_value(J.near_far[b * 2 + 0], J.near_far[b * 2 + 1], b, k, p, J.D, hw, J.depth_inv, J.dv + i, J.nf);
}

// ---- the composite network's preparation (enerf_composite_prep, enerf_forward_composite): everything of a frame that depends on
// the cameras, near_far and the boxes alone, in ONE launch at the head of the frame, before the layers' chains part:
//   * every level's projection matrices (block 0, as above);
//   * level 0's depth planes of all 1 + L cascades, each with its own near_far row and plane count (B == 1);
//   * the ray index and count of every rendered level's L windows (k_window_ray_index's arithmetic).
// One block-range per job, each at most kCompositePrepJobBlocks blocks whose threads stride over the job's elements: a few
// hundred blocks in all whatever the image size.  No LDS, plain vector stores.  The device functions are the stand-alone
// kernels' (proj_one, depth_plane_value): identical bits.
constexpr int kCompositePrepCascades = 5;        // ENERF_MAX_FG_LAYERS + 1
constexpr int kCompositePrepWindows = 12;        // ENERF_MAX_LEVELS * ENERF_MAX_FG_LAYERS
constexpr int kCompositePrepJobBlocks = 32;

// ---- boxes that move (enerf_forward_composite_moving): the layers' sizes (w, h) are the host's and part of the plan, their positions
// (x, y) are two float32 per layer in input-image pixels that the kernels read themselves.  ONE function resolves a position, so every
// user gets the same bits: a non-finite value becomes 0, the value is truncated toward zero and clamped to [0, extent - size] (the
// clamp of enerf_outdoor/enerf.py:165-168); *changed is set if any of that changed the value.  extent >= size (the plan checks).
__device__ __forceinline__ int resolve_box_position(float v, int size, int extent, bool* changed) {
    const bool finite = fabsf(v) <= 3.402823466e38f;               // false for NaN and +-inf
    const float f = finite ? truncf(v) : 0.f;
    const float hi = (float)(extent - size);                       // extents < 2^24: exact
    const float c = fminf(fmaxf(f, 0.f), hi);
    *changed = !(c == v);
    return (int)c;
}
// the corner of the layer's window in a level's grid: (int)((float)xi * (float)scale), a float32 product without contraction, then
// truncation — scaled_box of frame.hip, (bbox * scale).int() of the reference.  `room` = grid extent - window extent >= 0: for the
// scales the cascade uses (powers of two) the corner never exceeds it; for any other scale the min keeps a rounded product inside.
__device__ __forceinline__ int scaled_box_corner(int xi, float scale, int room) {
    const int c = (int)((float)xi * scale);                        // (a lone product: nothing to contract it with)
    return c < room ? c : room;
}
constexpr int kWinTableInts = 3 * 2 * 4 * 2;     // int win[ENERF_MAX_LEVELS][volume | render][ENERF_MAX_FG_LAYERS][2]
__host__ __device__ inline int win_table_at(int level, int render, int layer) { return ((level * 2 + render) * 4 + layer) * 2; }
// what the preparation needs to resolve every window of a frame whose positions are on the device
struct MovingBoxes {
    const float* xy;                 // (L, 2) float32 on the device; nullptr: the windows are the job's scalars, as ever
    int* table;                      // the resolved corners, kWinTableInts ints (win_table_at); unrendered levels' render rows are 0
    int* flags;                      // (L): bit 0 = the position was changed by the resolution
    int* flags_out;                  // optional copy of the flags for the caller (nullptr: none)
    int L, num_levels, H, W;
    int bw[4], bh[4];                // the layers' sizes in input-image pixels
    float vscale[3], rscale[3];      // volume_scale / render_scale per level
    int vroom[3][4][2], rroom[3][4][2];   // grid extent - window extent per level and layer, (x, y); rroom < 0: the level is not rendered
};
__device__ __forceinline__ void resolve_window(const MovingBoxes& M, int level, int render, int l, int* x0, int* y0, bool* changed) {
    bool cx, cy;
    const int xi = resolve_box_position(M.xy[2 * l + 0], M.bw[l], M.W, &cx);
    const int yi = resolve_box_position(M.xy[2 * l + 1], M.bh[l], M.H, &cy);
    const float sc = render ? M.rscale[level] : M.vscale[level];
    const int* room = render ? M.rroom[level][l] : M.vroom[level][l];
    *x0 = scaled_box_corner(xi, sc, room[0]);
    *y0 = scaled_box_corner(yi, sc, room[1]);
    *changed = cx || cy;
}
// block 0 of a job with moving boxes: the table and the flags, plain stores
__device__ __forceinline__ void composite_prep_window_table(const MovingBoxes& M, int tid, int threads) {
    for (int e = tid; e < 3 * 2 * 4; e += threads) {
        const int level = e / 8, render = (e >> 2) & 1, l = e & 3;
        int x0 = 0, y0 = 0;
        bool changed;
        if (level < M.num_levels && l < M.L && !(render && M.rroom[level][l][0] < 0)) resolve_window(M, level, render, l, &x0, &y0, &changed);
        M.table[win_table_at(level, render, l)] = x0;
        M.table[win_table_at(level, render, l) + 1] = y0;
    }
    if (tid < M.L) {
        int x0, y0;
        bool changed;
        resolve_window(M, 0, 0, tid, &x0, &y0, &changed);
        M.flags[tid] = changed ? 1 : 0;
        if (M.flags_out != nullptr) M.flags_out[tid] = changed ? 1 : 0;
    }
}

struct CompositePrep {
    ProjJob pj[3];                                // proj == nullptr: none
    struct Planes { const float* near_far; float *dv, *nf; int D, block0, blocks; } cas[kCompositePrepCascades];
    int n_cas, h, w, depth_inv;
    struct Window { int x0, y0, ww, wh, Wr, block0, blocks; int *index, *count; int level, layer; } win[kCompositePrepWindows];
    int n_win;
    int nblocks;
    // A cached frame (enerf_forward_composite_cached, enerf_composite_prep_indexed): the source cameras sit in a cache's tables behind a
    // device-side index.  pj[*].src_exts / src_ixts are then the (V,4,4) / (V,3,3) tables, source camera s is their row view_idx[s],
    // and block 0 also leaves the S gathered rows in cam_exts (S,4,4) / cam_ixts (S,3,3) for the raw renders.  An index outside [0,V)
    // is never used as an address: that camera's rows and matrices are NaN, and *invalid (optional) is 1 instead of 0: the frame's
    // merges then write NaN (k_composite_layers).  view_idx == nullptr: rows 0 .. S-1 as they are, as ever.
    const int* view_idx;
    int V;
    float *cam_exts, *cam_ixts;
    int* invalid;
    // Moving boxes (enerf_forward_composite_moving): mv.xy != nullptr.  A block that writes a window's ray list resolves the window
    // itself (resolve_window: a handful of integer operations, no exchange between blocks), block 0 also writes the table the
    // frame's windowed kernels read and the flags.  mv.xy == nullptr: x0, y0 of every Window as given.
    MovingBoxes mv;
};
inline int composite_prep_job_blocks(long long elements, int threads) {
    const long long nb = (elements + threads - 1) / threads;
    return (int)(nb < 1 ? 1 : nb > kCompositePrepJobBlocks ? kCompositePrepJobBlocks : nb);
}
// block 0 of an indexed job: the projection matrices from the indexed rows, and the rows themselves
__device__ __forceinline__ void composite_prep_indexed_cameras(const CompositePrep& J, int tid, int threads) {
    const float qnan = __int_as_float(0x7fc00000);
#pragma unroll 1
    for (int l = 0; l < 3; ++l) {
        const ProjJob& pj = J.pj[l];
        if (pj.proj == nullptr) continue;
        for (int q = tid; q < pj.S; q += threads) {
            const int v = J.view_idx[q];
            if (v >= 0 && v < J.V)      // (row v as "camera 0" of a one-camera table: proj_one's arithmetic, so its bits)
                proj_one(0, pj.src_ixts + (long long)v * 9, pj.src_exts + (long long)v * 16, pj.tar_ixt, pj.tar_ext, pj.S, pj.src_scale,
                         pj.tar_scale, pj.proj + q * 12);
            else
                for (int k = 0; k < 12; ++k) pj.proj[q * 12 + k] = qnan;
        }
    }
    const int S = J.pj[0].S;
    if (tid == 0 && J.invalid != nullptr) {
        int bad = 0;
        for (int q = 0; q < S; ++q) bad |= (J.view_idx[q] < 0 || J.view_idx[q] >= J.V) ? 1 : 0;
        J.invalid[0] = bad;
    }
    for (int i = tid; i < S * 25; i += threads) {
        const int q = i / 25, t = i - q * 25;
        const int v = J.view_idx[q];
        const bool ok = v >= 0 && v < J.V;
        if (t < 16) J.cam_exts[q * 16 + t] = ok ? J.pj[0].src_exts[(long long)v * 16 + t] : qnan;
        else J.cam_ixts[q * 9 + (t - 16)] = ok ? J.pj[0].src_ixts[(long long)v * 9 + (t - 16)] : qnan;
    }
}
__device__ __forceinline__ void composite_prep_block(const CompositePrep& J, int vb, int tid, int threads) {
    if (vb == 0 && J.view_idx != nullptr) composite_prep_indexed_cameras(J, tid, threads);
    else if (vb == 0) {
#pragma unroll 1
        for (int l = 0; l < 3; ++l)
            if (J.pj[l].proj != nullptr)
                for (int q = tid; q < J.pj[l].S; q += threads)
                    proj_one(q, J.pj[l].src_ixts, J.pj[l].src_exts, J.pj[l].tar_ixt, J.pj[l].tar_ext, J.pj[l].S, J.pj[l].src_scale,
                             J.pj[l].tar_scale, J.pj[l].proj);
    }
    if (vb == 0 && J.mv.xy != nullptr) composite_prep_window_table(J.mv, tid, threads);
    const int hw = J.h * J.w;
#pragma unroll 1
    for (int c = 0; c < J.n_cas; ++c) {
        const CompositePrep::Planes& P = J.cas[c];
        if (vb < P.block0 || vb >= P.block0 + P.blocks) continue;
        const float nn = P.near_far[0], ff = P.near_far[1];
        for (int i = (vb - P.block0) * threads + tid; i < P.D * hw; i += P.blocks * threads) {
            const int k = i / hw, p = i - k * hw;
            depth_plane_value(nn, ff, 0, k, p, P.D, hw, J.depth_inv, P.dv + i, P.nf);
        }
        return;
    }
#pragma unroll 1
    for (int j = 0; j < J.n_win; ++j) {
        const CompositePrep::Window& Wn = J.win[j];
        if (vb < Wn.block0 || vb >= Wn.block0 + Wn.blocks) continue;
        if (vb == Wn.block0 && tid == 0) Wn.count[0] = Wn.ww * Wn.wh;
        int x0 = Wn.x0, y0 = Wn.y0;
        if (J.mv.xy != nullptr) {                                   // uniform
            bool changed;
            resolve_window(J.mv, Wn.level, 1, Wn.layer, &x0, &y0, &changed);
        }
        for (int i = (vb - Wn.block0) * threads + tid; i < Wn.ww * Wn.wh; i += Wn.blocks * threads) {
            const int yy = i / Wn.ww, xx = i - yy * Wn.ww;
            Wn.index[i] = (y0 + yy) * Wn.Wr + x0 + xx;
        }
        return;
    }
}

}  // namespace enerf
