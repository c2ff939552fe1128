// composite_layers_body.h — the body of k_composite_layers<NFP> and of k_composite_layers_at<NFP> (composite_layers.h), included once
// into each: the two kernels differ in where a window's corner comes from and in nothing else, and the text they share is this file,
// so the kernel with the corners in its argument block compiles from the tokens it always had.  The including kernel defines
//   ENERF_CL_WIN_X(l), ENERF_CL_WIN_Y(l)   the corner of layer l's window: a.win[l][0..1], or the device table's entry
// and has `a` (CompositeLayers), `invalid` and the template value NFP in scope.  No include guard: it is included twice.
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= a.H * a.W) return;
    const int y = p / a.W, x = p - y * a.W;
    const int Ns = a.Ns, nf = a.L * Ns, T = nf + Ns;
    if (invalid != nullptr && invalid[0] != 0) {        // uniform
        const float qnan = __int_as_float(0x7fc00000);
        for (int i = 0; i < nf; ++i) a.z_vals[(long long)p * nf + i] = qnan;
        for (int t = 0; t < T; ++t) {
            *reinterpret_cast<float4*>(a.net_output + ((long long)p * T + t) * 4) = make_float4(qnan, qnan, qnan, qnan);
            a.weights[(long long)p * T + t] = qnan;
        }
        a.rgb[(long long)p * 3 + 0] = qnan; a.rgb[(long long)p * 3 + 1] = qnan; a.rgb[(long long)p * 3 + 2] = qnan;
        a.depth[p] = qnan;
        return;
    }
    int base[ENERF_MAX_FG_LAYERS];                      // the pixel's row in layer l's buffers, or -1
#pragma unroll
    for (int l = 0; l < ENERF_MAX_FG_LAYERS; ++l) {
        const int wx = ENERF_CL_WIN_X(l), wy = ENERF_CL_WIN_Y(l), ww = a.win[l][2], wh = a.win[l][3];
        base[l] = (l < a.L && x >= wx && x < wx + ww && y >= wy && y < wy + wh) ? (y - wy) * ww + (x - wx) : -1;
    }
    auto row_of = [&](int l) { return l == 0 ? base[0] : (l == 1 ? base[1] : (l == 2 ? base[2] : base[3])); };
    auto z_of = [&](int l) { return l == 0 ? a.fg_z[0] : (l == 1 ? a.fg_z[1] : (l == 2 ? a.fg_z[2] : a.fg_z[3])); };
    auto raw_of = [&](int l) { return l == 0 ? a.fg_raw[0] : (l == 1 ? a.fg_raw[1] : (l == 2 ? a.fg_raw[2] : a.fg_raw[3])); };
    float zk[NFP];
    int id[NFP];                                        // l * Ns + k of the sample in the slot
#pragma unroll
    for (int i = 0; i < NFP; ++i) {
        zk[i] = INFINITY;
        id[i] = i;
        if (i < nf) {
            const int l = i / Ns, k = i - l * Ns, row = row_of(l);
            zk[i] = row >= 0 ? z_of(l)[(long long)row * Ns + k] : 0.f;
            a.z_vals[(long long)p * nf + i] = zk[i];    // z_vals_ori: concatenation order
        }
    }
    if (a.L > 1) {                                      // uniform
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
    // alpha compositing (utils.py:922-933): no softmax of the weights
    float Tacc = 1.f, rgb0 = 0.f, rgb1 = 0.f, rgb2 = 0.f, dep = 0.f, acc = 0.f;
    auto step = [&](int t, const float4 c, float z) {
        *reinterpret_cast<float4*>(a.net_output + ((long long)p * T + t) * 4) = c;
        const float alpha = 1.f - expf(-c.w);
        const float wgt = alpha * Tacc;
        Tacc *= (1.f - alpha + 1e-10f);
        rgb0 += wgt * c.x; rgb1 += wgt * c.y; rgb2 += wgt * c.z;
        dep += wgt * z;
        acc += wgt;
        a.weights[(long long)p * T + t] = wgt;
    };
#pragma unroll
    for (int i = 0; i < NFP; ++i)
        if (i < nf) {
            const int l = id[i] / Ns, k = id[i] - l * Ns, row = row_of(l);
            float4 c = make_float4(0.f, 0.f, 0.f, 0.f);
            if (row >= 0) c = *reinterpret_cast<const float4*>(raw_of(l) + ((long long)row * Ns + k) * 4);
            step(i, c, zk[i]);
        }
    for (int k = 0; k < Ns; ++k)
        step(nf + k, *reinterpret_cast<const float4*>(a.bg_raw + ((long long)p * Ns + k) * 4), a.bg_z[(long long)p * Ns + k]);
    if (a.white_bkgd) { rgb0 += 1.f - acc; rgb1 += 1.f - acc; rgb2 += 1.f - acc; }
    a.rgb[(long long)p * 3 + 0] = rgb0; a.rgb[(long long)p * 3 + 1] = rgb1; a.rgb[(long long)p * 3 + 2] = rgb2;
    a.depth[p] = dep;
