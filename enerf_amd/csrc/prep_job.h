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
struct CompositePrep {
    ProjJob pj[3];                                // proj == nullptr: none
    struct Planes { const float* near_far; float *dv, *nf; int D, block0, blocks; } cas[kCompositePrepCascades];
    int n_cas, h, w, depth_inv;
    struct Window { int x0, y0, ww, wh, Wr, block0, blocks; int *index, *count; } win[kCompositePrepWindows];
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
        for (int i = (vb - Wn.block0) * threads + tid; i < Wn.ww * Wn.wh; i += Wn.blocks * threads) {
            const int yy = i / Wn.ww, xx = i - yy * Wn.ww;
            Wn.index[i] = (Wn.y0 + yy) * Wn.Wr + Wn.x0 + xx;
        }
        return;
    }
}

}  // namespace enerf
