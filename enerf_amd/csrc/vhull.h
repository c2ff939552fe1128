// vhull.h — the foreground's world-space box of a time frame, carved from the V masks on the device (included by io.hip).
//
// The reference loads this box from files another tool made (enerf_outdoor/enerf.py:64 and enerf_path.py:65 read
// vhull/{frame:06d}.npy, zjumocap reads fitted SMPL vertices); a frame that has just come off a camera has neither.  The model is the
// specification and stands in full in include/enerf_hip.h (enerf_vhull_bounds).  In short, all coordinates double:
//   voxel (i,j,k) of the grid over scene_bounds has the centre p = lo + (idx + 0.5) (hi - lo) / G;  view v: c = R p + t, abstains if
//   !(c.z > 0);  u = fx c.x / c.z + cx, v = fy c.y / c.z + cy (no skew), iu = floor(u + 0.5), iv = floor(v + 0.5), abstains if the pixel
//   is not inside the mask (tested in double BEFORE any conversion to int);  else m = masks[v,iv,iu] votes inside layer l iff
//   m == l + 1 (labels) or m != 0 (no labels, L = 1), and outside otherwise;  occupied_l <=> inside_l >= min_views && outside_l <= max_miss;
//   per layer the occupied index range gives bounds, counts, flags and corners.
//
// k_vhull_carve: 256 threads, a grid capped at kVhBlocksPerCu blocks per CU, every wave looping over RUNS — 64 voxels along x at one
// (j, k), lane = voxel, so the occupancy bytes of a run are one coalesced store and neighbouring lanes gather neighbouring mask pixels.
// A view's 12 + 4 camera numbers are converted to double once per block into LDS (every lane reads the same word: a broadcast).  A
// voxel's loop over the views ends as soon as its fate is sealed for every layer — too many outside votes, too few views left to reach
// min_views, or enough inside votes and too few views left to exceed max_miss — which changes the work, never the result; the loop is
// per lane (no cross-lane operation in it), so a wave runs until its last open voxel is sealed and sealed lanes issue no loads.
// Reduction: every lane keeps the integer min / max of its occupied voxels' indices and their count per layer over all its runs; one
// xor-shuffle tree per wave at the end, four waves through LDS, then ONE set of integer atomics per block and layer.  Integer
// min / max / add do not depend on order: the result is a function of the inputs alone.
// The accumulators (8 ints per layer in the workspace) are encoded so that ZERO means "nothing yet" and atomicMin alone maintains
// both ends of a range: lo[a] holds imin - G[a] (< 0), hi[a] holds -(imax + 1) (< 0); the count is an atomicAdd.  A fill kernel in
// front of the carving clears them, as part of the enqueued work: a captured replay starts clean and the workspace's earlier contents
// never show.  k_vhull_finish (one wave; lane 8 l + c = corner c of layer l) turns them into bounds, counts, flags and corners in
// double, without fused multiply-adds, rounded once to float32.

namespace enerf {

constexpr int kVhThreads = 256, kVhWaves = kVhThreads / kWave, kVhBlocksPerCu = 8;
constexpr int kVhAcc = 8;                                    // ints per layer: lo[3], hi[3], count, one of padding
constexpr int kVhVals = 7;                                   // of which reduced
constexpr int kVhEmpty = 0x7fffffff;

struct VhullGeom {
    double lo[3], ext[3];                                    // the scene box's min corner and hi - lo
    float box[6];                                            // scene_bounds as given
    int G[3];
    int V, H, W, min_views, max_miss;
    int nxr, nruns;                                          // runs along x; runs in all
};

__device__ __forceinline__ double vh_mul(double a, double b) {
#ifdef ENERF_EMU
    return a * b;
#else
    return __dmul_rn(a, b);
#endif
}
__device__ __forceinline__ double vh_add(double a, double b) {
#ifdef ENERF_EMU
    return a + b;
#else
    return __dadd_rn(a, b);
#endif
}

template <int L, bool LABELS>
__global__ __launch_bounds__(kVhThreads) void k_vhull_carve(const unsigned char* __restrict__ masks, const float* __restrict__ exts,
                                                            const float* __restrict__ ixts, VhullGeom g,
                                                            unsigned char* __restrict__ occupancy, int* __restrict__ acc) {
    __shared__ double s_cam[ENERF_VHULL_MAX_VIEWS * 16];      // per view: rows 0..2 of ext (R | t), fx, cx, fy, cy
    __shared__ int s_red[kVhWaves * ENERF_MAX_FG_LAYERS * kVhVals];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    for (int e = tid; e < g.V * 16; e += kVhThreads) {
        const int v = e >> 4, q = e & 15;
        const int kq = q == 12 ? 0 : (q == 13 ? 2 : (q == 14 ? 4 : 5));
        s_cam[e] = (double)(q < 12 ? exts[v * 16 + q] : ixts[v * 9 + kq]);
    }
    __syncthreads();

    int rlo[L][3], rhi[L][3], cnt[L];
#pragma unroll
    for (int l = 0; l < L; ++l) {
        cnt[l] = 0;
#pragma unroll
        for (int a = 0; a < 3; ++a) { rlo[l][a] = kVhEmpty; rhi[l][a] = -1; }
    }
    const int Gx = g.G[0], Gy = g.G[1];
    const double fW = (double)g.W, fH = (double)g.H;
    const long long hw = (long long)g.H * g.W;
    const int bid = (int)xcd_contiguous(blockIdx.x, gridDim.x);
    for (int run = bid * kVhWaves + wave; run < g.nruns; run += (int)gridDim.x * kVhWaves) {
        const int xr = run % g.nxr, jk = run / g.nxr, j = jk % Gy, k = jk / Gy;
        const int i = xr * kWave + lane;
        if (i >= Gx) continue;                                // (a ragged run's tail; no cross-lane operation follows in the loop)
        const double px = g.lo[0] + ((double)i + 0.5) * g.ext[0] / (double)g.G[0];
        const double py = g.lo[1] + ((double)j + 0.5) * g.ext[1] / (double)g.G[1];
        const double pz = g.lo[2] + ((double)k + 0.5) * g.ext[2] / (double)g.G[2];
        int votes = 0, inside[L];
#pragma unroll
        for (int l = 0; l < L; ++l) inside[l] = 0;
        for (int v = 0; v < g.V; ++v) {
            const double* c = s_cam + v * 16;
            const double cz = c[8] * px + c[9] * py + c[10] * pz + c[11];
            if (cz > 0.0) {                                   // (NaN abstains)
                const double cx = c[0] * px + c[1] * py + c[2] * pz + c[3];
                const double cy = c[4] * px + c[5] * py + c[6] * pz + c[7];
                const double fu = floor(c[12] * cx / cz + c[13] + 0.5), fv = floor(c[14] * cy / cz + c[15] + 0.5);
                if (fu >= 0.0 && fu < fW && fv >= 0.0 && fv < fH) {          // in double, before any int: NaN and inf abstain
                    const unsigned m = masks[(long long)v * hw + (long long)(int)fv * g.W + (int)fu];
                    ++votes;
#pragma unroll
                    for (int l = 0; l < L; ++l) inside[l] += (LABELS ? m == (unsigned)(l + 1) : m != 0u) ? 1 : 0;
                }
            }
            const int rem = g.V - 1 - v;                      // views still to vote
            bool open = false;
#pragma unroll
            for (int l = 0; l < L; ++l) {
                const int outside = votes - inside[l];
                const bool dead = outside > g.max_miss || inside[l] + rem < g.min_views;
                const bool kept = inside[l] >= g.min_views && outside + rem <= g.max_miss;
                open = open || !(dead || kept);
            }
            if (!open) break;
        }
        unsigned occ = 0;
#pragma unroll
        for (int l = 0; l < L; ++l) {
            if (inside[l] >= g.min_views && votes - inside[l] <= g.max_miss) {
                occ |= 1u << l;
                ++cnt[l];
                rlo[l][0] = min(rlo[l][0], i); rhi[l][0] = max(rhi[l][0], i);
                rlo[l][1] = min(rlo[l][1], j); rhi[l][1] = max(rhi[l][1], j);
                rlo[l][2] = min(rlo[l][2], k); rhi[l][2] = max(rhi[l][2], k);
            }
        }
        if (occupancy != nullptr) occupancy[((long long)k * Gy + j) * Gx + i] = (unsigned char)occ;
    }

    // the wave's ranges and counts, then the block's
#pragma unroll
    for (int l = 0; l < L; ++l) {
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                rlo[l][a] = min(rlo[l][a], __shfl_xor(rlo[l][a], m));
                rhi[l][a] = max(rhi[l][a], __shfl_xor(rhi[l][a], m));
            }
            cnt[l] += __shfl_xor(cnt[l], m);
        }
        if (lane == 0) {
            int* r = s_red + (wave * ENERF_MAX_FG_LAYERS + l) * kVhVals;
#pragma unroll
            for (int a = 0; a < 3; ++a) { r[a] = rlo[l][a]; r[3 + a] = rhi[l][a]; }
            r[6] = cnt[l];
        }
    }
    __syncthreads();
    if (tid >= L * kVhVals) return;
    const int l = tid / kVhVals, q = tid - l * kVhVals;
    int val = s_red[l * kVhVals + q];
    for (int w = 1; w < kVhWaves; ++w) {
        const int o = s_red[(w * ENERF_MAX_FG_LAYERS + l) * kVhVals + q];
        val = q < 3 ? min(val, o) : (q < 6 ? max(val, o) : val + o);
    }
    int* a = acc + l * kVhAcc + q;
    if (q < 3) {
        const int G = q == 0 ? g.G[0] : (q == 1 ? g.G[1] : g.G[2]);
        if (val != kVhEmpty) atomicMin(a, val - G);
    } else if (q < 6) {
        if (val >= 0) atomicMin(a, -(val + 1));
    } else if (val != 0) {
        atomicAdd(reinterpret_cast<unsigned*>(a), (unsigned)val);
    }
}

__global__ __launch_bounds__(64) void k_vhull_finish(const int* __restrict__ acc, VhullGeom g, double pad, int L,
                                                     float* __restrict__ bounds, int* __restrict__ counts, int* __restrict__ flags,
                                                     float* __restrict__ corners) {
    const int l = threadIdx.x >> 3, c = threadIdx.x & 7;
    if (l >= L) return;
    const int* a = acc + l * kVhAcc;
    const int n = a[6];
    float b[6];
    int f = 0;
    if (n == 0) {
        f = 1;
#pragma unroll
        for (int q = 0; q < 6; ++q) b[q] = g.box[q];
    } else {
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) {
            const int imin = a[ax] + g.G[ax], imax = -a[3 + ax] - 1;
            const double cell = g.ext[ax] / (double)g.G[ax];
            b[ax] = (float)vh_add(vh_add(g.lo[ax], vh_mul((double)imin, cell)), -pad);
            b[3 + ax] = (float)vh_add(vh_add(g.lo[ax], vh_mul((double)(imax + 1), cell)), pad);
            if (imin == 0 || imax == g.G[ax] - 1) f |= 2;
        }
    }
    float* o = corners + (l * 8 + c) * 3;                    // base_utils.get_bound_corners: x by bit 2 of c, y by bit 1, z by bit 0
    o[0] = (c & 4) ? b[3] : b[0];
    o[1] = (c & 2) ? b[4] : b[1];
    o[2] = (c & 1) ? b[5] : b[2];
    if (c != 0) return;
#pragma unroll
    for (int q = 0; q < 6; ++q) bounds[l * 6 + q] = b[q];
    counts[l] = n;
    flags[l] = f;
}

size_t vhull_workspace_bytes(int L) { return (size_t)L * kVhAcc * sizeof(int); }

void launch_vhull_bounds(const enerf_vhull_t& a, hipStream_t st) {
    VhullGeom g;
    for (int ax = 0; ax < 3; ++ax) {
        g.lo[ax] = (double)a.scene_bounds[0][ax];
        g.ext[ax] = (double)a.scene_bounds[1][ax] - (double)a.scene_bounds[0][ax];
        g.box[ax] = a.scene_bounds[0][ax];
        g.box[3 + ax] = a.scene_bounds[1][ax];
        g.G[ax] = a.grid[ax];
    }
    g.V = a.V; g.H = a.H; g.W = a.W; g.min_views = a.min_views; g.max_miss = a.max_miss;
    g.nxr = cdiv(a.grid[0], kWave);
    g.nruns = g.nxr * a.grid[1] * a.grid[2];                  // <= 4 * 256 * 256
    const int L = a.n_layers;
    int* acc = (int*)a.workspace;
    zero_async(acc, vhull_workspace_bytes(L), st);
    const unsigned blocks = (unsigned)min(cdiv(g.nruns, kVhWaves), device_cu_count() * kVhBlocksPerCu);
    if (!a.labels) ENERF_LAUNCH((k_vhull_carve<1, false>), blocks, kVhThreads, 0, st, a.masks, a.exts, a.ixts, g, a.occupancy, acc);
    else if (L == 1) ENERF_LAUNCH((k_vhull_carve<1, true>), blocks, kVhThreads, 0, st, a.masks, a.exts, a.ixts, g, a.occupancy, acc);
    else if (L == 2) ENERF_LAUNCH((k_vhull_carve<2, true>), blocks, kVhThreads, 0, st, a.masks, a.exts, a.ixts, g, a.occupancy, acc);
    else if (L == 3) ENERF_LAUNCH((k_vhull_carve<3, true>), blocks, kVhThreads, 0, st, a.masks, a.exts, a.ixts, g, a.occupancy, acc);
    else ENERF_LAUNCH((k_vhull_carve<4, true>), blocks, kVhThreads, 0, st, a.masks, a.exts, a.ixts, g, a.occupancy, acc);
    ENERF_LAUNCH_SIMPLE(k_vhull_finish, 1u, 64, 0, st, acc, g, a.pad, L, a.bounds, a.counts, a.flags, a.corners);
}

}  // namespace enerf

extern "C" {

size_t enerf_vhull_workspace_bytes(const enerf_vhull_t* args) {
    if (args == nullptr) { enerf::fail(ENERF_EINVAL, "vhull_workspace_bytes: null args"); return 0; }
    if (args->n_layers < 1 || args->n_layers > ENERF_MAX_FG_LAYERS) {
        enerf::fail(ENERF_EINVAL, "vhull_workspace_bytes: L=%d foreground layers unsupported (1..%d)", args->n_layers, ENERF_MAX_FG_LAYERS);
        return 0;
    }
    return enerf::vhull_workspace_bytes(args->n_layers);
}

int enerf_vhull_bounds(const enerf_vhull_t* args, enerf_stream_t stream) {
    REQUIRE(args != nullptr, "vhull_bounds: null args");
    const enerf_vhull_t& a = *args;
    REQUIRE(a.masks && a.exts && a.ixts, "vhull_bounds: null %s", !a.masks ? "masks" : (!a.exts ? "exts" : "ixts"));
    REQUIRE(a.bounds && a.counts && a.flags && a.corners, "vhull_bounds: null %s",
            !a.bounds ? "bounds" : (!a.counts ? "counts" : (!a.flags ? "flags" : "corners")));
    REQUIRE(a.V >= 1 && a.V <= ENERF_VHULL_MAX_VIEWS, "vhull_bounds: V=%d views (1..%d)", a.V, ENERF_VHULL_MAX_VIEWS);
    REQUIRE(a.H >= 1 && a.W >= 1 && a.H <= 32768 && a.W <= 32768, "vhull_bounds: bad mask extent %dx%d (1..32768)", a.H, a.W);
    for (int ax = 0; ax < 3; ++ax)
        REQUIRE(a.grid[ax] >= 1 && a.grid[ax] <= 256, "vhull_bounds: grid (%d,%d,%d), every extent in 1..256", a.grid[0], a.grid[1], a.grid[2]);
    REQUIRE(a.n_layers >= 1 && a.n_layers <= ENERF_MAX_FG_LAYERS, "vhull_bounds: L=%d foreground layers unsupported (1..%d)", a.n_layers,
            ENERF_MAX_FG_LAYERS);
    REQUIRE(a.labels != 0 || a.n_layers == 1, "vhull_bounds: L=%d layers need labels (without labels L must be 1)", a.n_layers);
    REQUIRE(a.min_views >= 1, "vhull_bounds: min_views=%d (>= 1)", a.min_views);
    REQUIRE(a.max_miss >= 0, "vhull_bounds: max_miss=%d (>= 0)", a.max_miss);
    REQUIRE(a.pad >= 0.0 && a.pad <= 3.0e38, "vhull_bounds: pad=%g (finite, >= 0)", a.pad);                 // (NaN fails too)
    for (int ax = 0; ax < 3; ++ax) {
        const float lo = a.scene_bounds[0][ax], hi = a.scene_bounds[1][ax];
        REQUIRE(lo < hi && lo >= -3.0e38f && hi <= 3.0e38f, "vhull_bounds: scene_bounds axis %d is [%g, %g] (finite, lo < hi)", ax, lo, hi);
    }
    REQUIRE(a.workspace != nullptr, "vhull_bounds: null workspace");
    REQUIRE(((size_t)a.workspace & 3) == 0, "vhull_bounds: workspace is not 4-byte aligned");
    REQUIRE(a.workspace_bytes >= enerf::vhull_workspace_bytes(a.n_layers), "vhull_bounds: workspace of %zu bytes, %zu needed",
            a.workspace_bytes, enerf::vhull_workspace_bytes(a.n_layers));
    enerf::launch_vhull_bounds(a, (hipStream_t)stream);
    return enerf::check_launch("vhull_bounds");
}

}  // extern "C"
