"""Cases of the composite network's kernels (csrc/composite_layers.h, k_feature_volume_mp<CQ, true>, k_render_rays<..., RAW>),
shared by the emulator tests (test_composite.py) and the MI355X tests (test_composite_gpu.py): every function takes the library
and the device and asserts.

    window_volume_case        the windowed cost volume is the full one, sliced, bit for bit
    window_regression_case    the windowed regression is the plain regression of the zero-padded prob, bit for bit
    raw_render_case           raw samples [r, g, b, sigma] and their depths against the float64 oracle of test_render_regimes.py
                              (its inputs, its bound: e_hip <= max(TAU, 3 e_ref)); vol = NULL is vol of zeros, bit for bit
    raw_selection_case        a window's rays picked by the device index list = a render of the gathered rays, bit for bit
    composite_case            the layer merge + composite against composite_reference (float64), 1e-5 of the largest value
"""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

from enerf_amd.config import EnerfConfig
from enerf_amd.synth import make_batch

# (x0, y0, ww, wh) in the 8 x 12 (h x w) grid: two that touch edges and overlap each other, one with odd offsets, the whole grid
GRID_H, GRID_W = 8, 12
WINDOWS = [(4, 0, 8, 8), (0, 0, 8, 4), (3, 2, 4, 4), (0, 0, GRID_W, GRID_H)]


def _same(a, b, what):
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert torch.equal(a, b), (what, float((a - b).abs().max()))


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. windowed cost volume
def window_volume_case(lib, dev, C):
    S, D, h, w = 2, 4, GRID_H, GRID_W
    cas = EnerfConfig().cas
    batch = {k: torch.from_numpy(v).to(dev) for k, v in make_batch(4 * h, 4 * w, S, EnerfConfig(), seed=11, B=1).items()}
    g = torch.Generator().manual_seed(100 + C)
    feat = torch.randn(1, S, h, w, C, generator=g).to(dev)
    near, far = float(batch["near_far"][0, 0]), float(batch["near_far"][0, 1])
    dv = (near + (far - near) * torch.rand(1, D, h, w, generator=g)).to(dev)          # per-pixel planes: a shifted window would show
    proj = lib.get_proj_mats(batch["src_ixts"], batch["src_exts"], batch["tar_ixt"], batch["tar_ext"], cas.im_feat_scale[0], cas.volume_scale[0])
    full = lib.build_feature_volume(feat, proj, dv, C)
    assert float(full.abs().max()) > 0
    for win in WINDOWS:
        x0, y0, ww, wh = win
        got = lib.build_feature_volume_window(feat, proj, dv, C, win)
        _same(got, full[:, :, y0:y0 + wh, x0:x0 + ww].contiguous(), ("vol_window", C, win))


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. windowed depth regression
def window_regression_case(lib, dev, D, depth_inv):
    h, w = GRID_H, GRID_W
    g = torch.Generator().manual_seed(200 + D + int(depth_inv))
    dv = (0.3 + 2.0 * torch.rand(1, D, h, w, generator=g)).to(dev)
    for win in WINDOWS:
        x0, y0, ww, wh = win
        prob = (3.0 * torch.randn(1, D, wh, ww, generator=g)).to(dev)
        padded = torch.zeros(1, D, h, w, device=dev)
        padded[:, :, y0:y0 + wh, x0:x0 + ww] = prob
        want = lib.depth_regression(padded, dv, depth_inv)
        got = lib.depth_regression_window(prob, dv, depth_inv, win)
        for name, a, b in zip(("depth", "std"), got, want):
            _same(a, b, ("regression_window", name, D, depth_inv, win))
        # the pixel row just outside the window (above or below it): zero logits = a uniform softmax over the D planes
        for yo in (y0 - 1, y0 + wh):
            if 0 <= yo < h:
                v = dv[0, :, yo].double().cpu()
                v = 1.0 / v.clamp_min(1e-6) if depth_inv else v
                mu = v.mean(0)
                sd = ((v - mu) ** 2).mean(0).clamp_min(1e-10).sqrt()
                assert float((got[0][0, yo].double().cpu() - mu).abs().max()) <= 1e-6 * float(mu.abs().max()), (D, depth_inv, win, yo)
                assert float((got[1][0, yo].double().cpu() - sd).abs().max()) <= 1e-5 * float(sd.abs().max()), (D, depth_inv, win, yo)


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. raw-sample render
def _rr():
    import test_render_regimes as RR
    return RR


def _raw_oracle(RR, sd, level, S, rays12, vol, ns, dtype):
    """(raw (1,N,ns,4), z (1,N,ns) metric) of oracle.render_rays in ``dtype``, viewdir_agg off."""
    from oracle import enerf_oracle as O
    batch, feats = RR._scene(S, 1)
    cast = lambda t: t.to(dtype) if t.is_floating_point() else t
    cfg = EnerfConfig(viewdir_agg=False).with_cas(num_samples=(ns, ns))
    with torch.no_grad():
        out = O.render_rays(cfg, {k: cast(v) for k, v in sd.items()}, cast(rays12), level, {k: cast(v) for k, v in batch.items()},
                            cast(feats[f"level_{RR.CAS.render_im_feat_level[level]}"]), cast(vol), return_intermediates=True)
    z = out["_z"]
    return out["_raw"], (1.0 / z if RR.CAS.depth_inv[level] else z)          # network_composite.py:48-51


def _render_raw(RR, p, rays, ns, vol="given", **kw):
    level = p["level"]
    return p["lib"].render_rays_raw(rays.to(p["dev"]).contiguous(), p["tex"], p["vol"] if vol == "given" else vol, *p["cams"], p["packed"],
                                    n_samples=ns, depth_inv=RR.CAS.depth_inv[level], F=RR.CAS.nerf_model_feat_ch[level] + 3,
                                    render_scale=RR.CAS.render_scale[level], **kw)


def raw_render_case(lib, dev, gpu, level, S, ns, worst=None):
    """37 rays (two full 16-ray tiles and a ragged one); with the volume, and without it against a volume of zeros."""
    RR = _rr()
    net, sd = RR._net(False, gpu)
    x = RR._inputs(level, S, 1, 37, seed=3000 + 100 * level + 10 * S + ns)
    p = RR._prep(lib, dev, net, level, S, 1, x["vol"])
    tag = f"raw F={RR.CAS.nerf_model_feat_ch[level] + 3} S={S} Ns={ns}"
    for what, vol in (("vol", x["vol"]), ("zeros", torch.zeros_like(x["vol"]))):
        pz = p if what == "vol" else RR._prep(lib, dev, net, level, S, 1, vol)
        got = _render_raw(RR, pz, x["rays12"], ns)
        r64 = _raw_oracle(RR, sd, level, S, x["rays12"], vol, ns, torch.float64)
        r32 = _raw_oracle(RR, sd, level, S, x["rays12"], vol, ns, torch.float32)
        for name, hip, a, b in zip(("raw", "z"), got, r64, r32):
            assert hip.shape == a.shape, (tag, name, hip.shape, a.shape)
            scale = float(a.abs().max())
            e_hip, e_ref = float((hip.cpu().double() - a).abs().max()) / scale, float((b.double() - a).abs().max()) / scale
            print(f"[composite] {tag} {what} {name}: e_hip {e_hip:.2e} e_ref {e_ref:.2e}")
            if worst is not None:
                worst[name] = max(worst.get(name, 0.0), e_hip)
            assert e_hip <= max(RR.TAU, 3.0 * e_ref), f"{tag} {what}: {name} e_hip {e_hip:.3e} > max({RR.TAU:.0e}, 3 x e_ref {e_ref:.3e})"
        if what == "zeros":
            null = _render_raw(RR, pz, x["rays12"], ns, vol=None)
            _same(null[0], got[0], (tag, "vol NULL raw"))
            _same(null[1], got[1], (tag, "vol NULL z"))
    # the fused build_rays form (8-float rays + maps) gives the bits of the 12-float rays enerf_build_rays makes from them
    maps = tuple(m.to(dev) for m in x["maps"])
    Hr, Wr = p["tex"].shape[2:4]
    r12 = lib.build_rays(x["rays8"].to(dev), *maps, Hr, Wr, RR.CAS.depth_inv[level])
    a = _render_raw(RR, p, r12, ns)
    b = _render_raw(RR, p, x["rays8"], ns, maps=maps)
    _same(a[0], b[0], (tag, "maps raw"))
    _same(a[1], b[1], (tag, "maps z"))


def raw_selection_case(lib, dev, gpu, level):
    """A 5 x 7 window of a 12 x 16 ray raster through enerf_window_ray_index + the kernel's device-side selection: rows [0, 35) hold
    what a render of the gathered rays gives, the rows behind them keep the caller's sentinel."""
    RR = _rr()
    net, _ = RR._net(False, gpu)
    Hr, Wr, ns = 12, 16, 2
    win = (4, 3, 5, 7)
    x0, y0, ww, wh = win
    x = RR._inputs(level, 3, 1, Hr * Wr, seed=3500 + level)
    p = RR._prep(lib, dev, net, level, 3, 1, x["vol"])
    index, count = lib.window_ray_index(win, Hr, Wr, dev)
    want_idx = (torch.arange(y0, y0 + wh)[:, None] * Wr + torch.arange(x0, x0 + ww)[None]).reshape(-1)
    assert int(count.cpu()) == ww * wh and torch.equal(index.cpu().long()[:ww * wh], want_idx)
    want = _render_raw(RR, p, x["rays12"][:, want_idx], ns)
    full_index = torch.cat([index, torch.zeros(Hr * Wr - index.numel(), dtype=torch.int32, device=dev)])
    SENT = -7.0
    out = (torch.full((1, Hr * Wr, ns, 4), SENT, device=dev), torch.full((1, Hr * Wr, ns), SENT, device=dev))
    got = _render_raw(RR, p, x["rays12"], ns, ray_index=full_index, ray_count=count, out=out)
    n = ww * wh
    _same(got[0][:, :n], want[0], ("selection raw", level))
    _same(got[1][:, :n], want[1], ("selection z", level))
    assert bool((got[0][:, n:] == SENT).all()) and bool((got[1][:, n:] == SENT).all()), level
    # compact buffers of exactly the window's size (what the network allocates)
    small = _render_raw(RR, p, x["rays12"], ns, ray_index=index, ray_count=count, n_out=n)
    _same(small[0], want[0], ("selection raw compact", level))
    _same(small[1], want[1], ("selection z compact", level))


def raw_tile_walk_case(lib, dev, gpu, level, cus_list=()):
    """331 rays = 21 tiles.  Under ``emu_cu_count`` (the emulator only) the persistent launch shrinks to one or two blocks and every
    wave walks several tiles; the result must not change by a bit."""
    RR = _rr()
    net, _ = RR._net(False, gpu)
    ns = 2
    rays, vol = RR._bulk(level, 331, 3600 + level)
    p = RR._prep(lib, dev, net, level, 3, 1, vol)
    ref = _render_raw(RR, p, rays, ns)
    for mb in (1, 3):
        got = _render_raw(RR, p, rays, ns, max_blocks=mb)
        _same(got[0], ref[0], ("tile walk raw max_blocks", level, mb))
        _same(got[1], ref[1], ("tile walk z max_blocks", level, mb))
    if cus_list:
        from emu_lib import emu_cu_count
        for cus in cus_list:
            with emu_cu_count(lib, cus):
                got = _render_raw(RR, p, rays, ns)
            _same(got[0], ref[0], ("tile walk raw cus", level, cus))
            _same(got[1], ref[1], ("tile walk z cus", level, cus))


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. layer merge + composite
IMG_H, IMG_W = 6, 10
BOXES = {      # (x0, y0, ww, wh) in the 6 x 10 image
    (1, "interior"): [(2, 1, 5, 4)],
    (1, "corner"): [(7, 4, 3, 2)],
    (2, "overlapping"): [(0, 0, 6, 4), (3, 1, 6, 5)],
    (2, "disjoint"): [(0, 0, 4, 3), (5, 3, 5, 3)],
    (3, "overlapping+corner"): [(0, 0, 6, 4), (3, 1, 6, 5), (7, 4, 3, 2)],
    (3, "nested"): [(0, 0, 10, 6), (2, 1, 5, 4), (3, 2, 2, 2)],
}
COMPOSITE_CASES = [(L, name, ns) for (L, name) in BOXES for ns in (1, 2)]
COMPOSITE_TOL = 1e-5


def composite_reference(fg, windows, bg, H, W, white_bkgd=False):
    """parse_layer + raw2outputs_composite (utils.py:875-942) restated in the dtype of its inputs: scatter every layer into a full
    image of zero samples, concatenate, sort by depth when there is more than one layer (stable: equal depths keep the
    concatenation order), append the background, alpha-composite with no softmax of the weights."""
    bg_raw, bg_z = bg
    Ns = bg_z.shape[-1]
    nets, zs = [], []
    for (raw, z), (x0, y0, ww, wh) in zip(fg, windows):
        R = torch.zeros(H, W, Ns, 4, dtype=raw.dtype)
        Z = torch.zeros(H, W, Ns, dtype=raw.dtype)
        R[y0:y0 + wh, x0:x0 + ww] = raw.reshape(wh, ww, Ns, 4)
        Z[y0:y0 + wh, x0:x0 + ww] = z.reshape(wh, ww, Ns)
        nets.append(R.reshape(H * W, Ns, 4))
        zs.append(Z.reshape(H * W, Ns))
    net, z = torch.cat(nets, -2), torch.cat(zs, -1)
    z_ori = z
    if len(fg) > 1:
        z, idx = torch.sort(z, dim=-1, stable=True)
        net = net.gather(1, idx[..., None].repeat(1, 1, 4))
    net = torch.cat([net, bg_raw.reshape(H * W, Ns, 4)], -2)
    z = torch.cat([z, bg_z.reshape(H * W, Ns)], -1)
    alpha = 1.0 - torch.exp(-net[..., 3])
    T = torch.cumprod(1.0 - alpha + 1e-10, -1)[..., :-1]
    T = torch.cat([torch.ones_like(alpha[..., :1]), T], -1)
    weights = alpha * T
    rgb = torch.sum(weights[..., None] * net[..., :3], -2)
    depth = torch.sum(weights * z, -1)
    if white_bkgd:
        rgb = rgb + (1.0 - weights.sum(-1)[..., None])
    return {"rgb": rgb, "depth": depth, "weights": weights, "net_output": net, "z_vals": z_ori}


def composite_inputs(L, name, ns, seed=0):
    """fp32 CPU inputs: colours in [0, 1], sigma >= 0 with a fifth of the samples at exactly 0 and a fifth at 80 (1 - alpha and then
    the transmittance underflow in fp32), depths in per-layer ranges that interleave; on the pixels all of two layers cover, the
    second layer's depths EQUAL the first's and both have zero sigma (the tie the stable order decides)."""
    g = torch.Generator().manual_seed(seed + 1000 * L + 10 * ns + len(name))
    windows = BOXES[(L, name)]

    def samples(n, lo, hi):
        raw = torch.rand(n, ns, 4, generator=g)
        raw[..., 3] = -torch.log(torch.rand(n, ns, generator=g).clamp_min(1e-3)) * 2.0
        kind = torch.rand(n, ns, generator=g)
        raw[..., 3][kind < 0.2] = 0.0
        raw[..., 3][kind > 0.8] = 80.0
        z = lo + (hi - lo) * torch.rand(n, ns, generator=g)
        return raw, z

    fg = [samples(ww * wh, 1.0 + 0.3 * l, 3.0 + 0.3 * l) for l, (_, _, ww, wh) in enumerate(windows)]
    if L > 1:
        (ax, ay, aw, ah), (bx, by, bw, bh) = windows[0], windows[1]
        for y in range(max(ay, by), min(ay + ah, by + bh)):
            for x in range(max(ax, bx), min(ax + aw, bx + bw)):
                if (x + y) % 2 == 0:
                    ra, rb = (y - ay) * aw + (x - ax), (y - by) * bw + (x - bx)
                    fg[1][1][rb] = fg[0][1][ra]
                    fg[0][0][ra, :, 3] = 0.0
                    fg[1][0][rb, :, 3] = 0.0
    bg = samples(IMG_H * IMG_W, 4.0, 9.0)
    return fg, windows, bg


def composite_case(lib, dev, L, name, ns, worst=None):
    fg, windows, bg = composite_inputs(L, name, ns)
    to = lambda pair: tuple(t.to(dev).contiguous() for t in pair)
    for white in (False, True):
        got = lib.composite_layers([to(f) for f in fg], windows, to(bg), IMG_H, IMG_W, white_bkgd=white)
        again = lib.composite_layers([to(f) for f in fg], windows, to(bg), IMG_H, IMG_W, white_bkgd=white)
        ref = composite_reference([tuple(t.double() for t in f) for f in fg], windows, tuple(t.double() for t in bg), IMG_H, IMG_W, white)
        assert set(got) == set(ref)
        for k in ref:
            _same(got[k], again[k], ("composite twice", L, name, ns, k))
            h = got[k].cpu().double()
            assert h.shape == ref[k].shape, (k, h.shape, ref[k].shape)
            if k in ("net_output", "z_vals"):                       # data movement only: the order itself
                assert torch.equal(h, ref[k]), (L, name, ns, k)
                continue
            e = float((h - ref[k]).abs().max()) / float(ref[k].abs().max())
            print(f"[composite] L={L} {name} Ns={ns} white={int(white)} {k}: e {e:.2e}")
            if worst is not None:
                worst[k] = max(worst.get(k, 0.0), e)
            assert e <= COMPOSITE_TOL, (L, name, ns, white, k, e)
        if not white:
            assert float(got["weights"].sum(-1).max()) <= 1.0 + 1e-6


def composite_refusals(lib, dev):
    from enerf_amd.lib import EnerfError
    import pytest
    z4 = lambda n, ns: (torch.zeros(n, ns, 4, device=dev), torch.zeros(n, ns, device=dev))
    with pytest.raises(EnerfError, match="L\\*n_samples <= 16"):          # L * Ns = 20
        lib.composite_layers([z4(4, 5)] * 4, [(0, 0, 2, 2)] * 4, z4(IMG_H * IMG_W, 5), IMG_H, IMG_W)
    with pytest.raises(EnerfError, match="outside"):
        lib.composite_layers([z4(6, 1)], [(8, 4, 3, 2)], z4(IMG_H * IMG_W, 1), IMG_H, IMG_W)
    with pytest.raises(EnerfError):
        lib.composite_layers([z4(4, 1)] * 5, [(0, 0, 2, 2)] * 5, z4(IMG_H * IMG_W, 1), IMG_H, IMG_W)


def window_refusals(lib, dev):
    """Every new entry validates before it launches."""
    from enerf_amd.lib import EnerfError
    import pytest
    feat, proj = torch.zeros(1, 2, 8, 12, 16, device=dev), torch.zeros(1, 2, 3, 4, device=dev)
    dv = torch.ones(1, 4, 8, 12, device=dev)
    with pytest.raises(EnerfError, match="outside"):
        lib.build_feature_volume_window(feat, proj, dv, 16, (8, 0, 8, 8))
    with pytest.raises(EnerfError, match="divisible by 4"):
        lib.build_feature_volume_window(feat, proj, dv, 16, (0, 0, 6, 8))
    with pytest.raises(EnerfError, match="divisible by 4"):
        lib.build_feature_volume_window(feat, proj, torch.ones(1, 6, 8, 12, device=dev), 16, (0, 0, 8, 8))
    with pytest.raises(EnerfError, match="unsupported"):
        lib.build_feature_volume_window(torch.zeros(1, 2, 8, 12, 8, device=dev), proj, dv, 8, (0, 0, 8, 8))
    with pytest.raises(EnerfError, match="outside"):
        lib.depth_regression_window(torch.zeros(1, 4, 4, 4, device=dev), dv, False, (0, 6, 4, 4))
    with pytest.raises(EnerfError, match="divisible by 4"):
        lib.depth_regression_window(torch.zeros(1, 4, 4, 2, device=dev), dv, False, (0, 0, 2, 4))
    with pytest.raises(EnerfError, match="outside"):
        lib.window_ray_index((10, 0, 8, 4), 12, 16, dev)
    with pytest.raises(EnerfError, match="null pointer"):
        lib._check(lib.dll.enerf_window_ray_index(0, 0, 4, 4, 12, 16, None, None, None), "window_ray_index")
    with pytest.raises(EnerfError, match="null args"):
        lib._check(lib.dll.enerf_render_rays_raw(None, None), "render_rays_raw")
    with pytest.raises(EnerfError, match="null args"):
        lib._check(lib.dll.enerf_composite_layers(None, None), "composite_layers")


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. the whole network against the reference's fixtures (tools/make_golden_composite.py writes them, tests/golden/composite_*.npz)
GOLDEN = os.path.join(HERE, "golden")
REL_TOL = 1e-4            # the project's bar (tests/test_gpu_parity.py::REL_TOL)
# boxes: (x, y, w, h) in pixels of the 64 x 96 input image; ranges: per foreground layer, then the background, as fractions of the
# rig's [near, far].  Case "a": two layers that overlap on 32 x 32 pixels, one touching three image edges, a third of the image in
# no box; layer 0 has the FAR range, so the sorted order differs from the concatenation order wherever both cover a pixel.
# Case "b": one interior layer, last level only (level 0 only hands the padded regression's depth / std to level 1), no sort.
NETWORK_CASES = {
    "a": dict(H=64, W=96, S=3, L=2, render_if=(True, True), boxes=[(32, 0, 64, 64), (0, 0, 64, 32)],
              ranges=[(0.55, 0.85), (0.10, 0.40), (0.0, 1.0)], seed=21),
    "b": dict(H=64, W=96, S=2, L=1, render_if=(False, True), boxes=[(32, 16, 32, 32)], ranges=[(0.2, 0.7), (0.0, 1.0)], seed=22,
              drop=("_layer1.",)),
}
WEIGHT_FILES = "composite_weights_{}.npz"       # the two-layer network's state dict, split so that no file passes 1 MiB


def network_config(name):
    """enerf_outdoor/actor1.yaml's enerf block on its parent dtu_pretrain.yaml, with the case's render_if."""
    return EnerfConfig(viewdir_agg=False).with_cas(volume_planes=(32, 8), num_samples=(2, 1), render_if=NETWORK_CASES[name]["render_if"])


def network_batch(name):
    """The reference's batch as float32 numpy arrays: make_batch + bbox (1,L,4), per-layer near_far (1,L+1,2), seeded bg_src_inps."""
    import numpy as np
    c = NETWORK_CASES[name]
    b = make_batch(c["H"], c["W"], c["S"], network_config(name), seed=c["seed"], textured=True)
    n, f = float(b["near_far"][0, 0]), float(b["near_far"][0, 1])
    b["near_far"] = np.array([[(n + lo * (f - n), n + hi * (f - n)) for lo, hi in c["ranges"]]], np.float32)
    b["bbox"] = np.array([c["boxes"]], np.float32)
    b["bg_src_inps"] = np.random.default_rng(c["seed"] + 100).uniform(-1, 1, size=b["src_inps"].shape).astype(np.float32)
    return b


def network_weights(name):
    """The case's reference state dict: the stored two-layer one, minus the keys the case's rule drops."""
    import glob
    import numpy as np
    sd = {}
    for p in sorted(glob.glob(os.path.join(GOLDEN, WEIGHT_FILES.format("*")))):
        z = np.load(p)
        sd.update({k: torch.from_numpy(z[k]) for k in z.files})
    drop = NETWORK_CASES[name].get("drop", ())
    return {k: v for k, v in sd.items() if not any(d in k for d in drop)}


def network_case(lib, dev, name, worst=None):
    import numpy as np
    from enerf_amd.network_composite import Network
    c = NETWORK_CASES[name]
    gold = np.load(os.path.join(GOLDEN, f"composite_{name}.npz"))
    net = Network(network_config(name), c["L"], lib=lib)
    sd = network_weights(name)
    n_par = sum(p.numel() for p in net.parameters())
    assert (len(net.state_dict()), n_par) == {2: (440, 599330), 1: (324, 424460)}[c["L"]], (len(net.state_dict()), n_par)
    missing = net.load_state_dict(sd, strict=False)                 # (the fixtures leave out BatchNorm's batch counters)
    assert not missing.unexpected_keys and all(k.endswith("num_batches_tracked") for k in missing.missing_keys), missing
    full = dict(net.state_dict())
    full.update(sd)
    net.load_state_dict(full, strict=True)
    net = net.to(dev)
    import pytest
    with pytest.raises(RuntimeError, match="inference only"):
        net.train()(None)
    net.eval()
    batch = {k: torch.from_numpy(v).to(dev) for k, v in network_batch(name).items()}
    batch["bbox"] = batch["bbox"].cpu()
    with torch.no_grad():
        first = {k: v.clone() for k, v in net(batch).items()}
        out = net(batch)
        # buffers are per shape: a later frame of the shape allocates nothing, writes where the first one wrote, and gives its bits
        ptrs = {k: v.data_ptr() for k, v in out.items()}
        count = (lambda: torch.cuda.memory_stats(dev)["allocation.all.allocated"]) if dev.type == "cuda" else (lambda: 0)
        before = count()
        out = net(batch)
        assert count() == before, "a frame of a known shape allocated device memory"
        assert {k: v.data_ptr() for k, v in out.items()} == ptrs
        for k, v in out.items():
            assert torch.equal(v, first[k]), k
    got = {k: v for k, v in out.items()}
    got.update({f"mid/{k}": v for k, v in net.intermediates.items()})
    want = {k: gold[k] for k in gold.files}
    assert set(got) == set(want), (sorted(set(got) ^ set(want)))
    assert not any(k.startswith("idx") for k in got)
    for k in sorted(want):
        a, b = got[k].cpu().double(), torch.from_numpy(want[k]).double()
        assert a.shape == b.shape, (k, a.shape, b.shape)
        e = float((a - b).abs().max()) / float(b.abs().max())
        print(f"[composite] case {name} {k}: e {e:.2e}")
        if worst is not None:
            key = k.split("/")[-1].split("_")[0]
            worst[key] = max(worst.get(key, 0.0), e)
        assert e <= REL_TOL, (name, k, e)
    H, W = c["H"], c["W"]
    for i, on in enumerate(c["render_if"]):
        if not on:
            assert f"rgb_level{i}" not in got
            continue
        rs = network_config(name).cas.render_scale[i]
        Hr, Wr = int(H * rs), int(W * rs)
        wsum = got[f"weights_level{i}"].sum(-1)
        assert float(wsum.max()) < 1.0 and float(wsum.min()) >= 0.0            # alpha compositing, no softmax (a softmax sums to 1)
        # outside every box the foreground samples are zeros: the pixel is the background's own composite
        free = torch.ones(Hr, Wr, dtype=torch.bool)
        for box in c["boxes"]:
            x, y, w, h = (int(v * rs) for v in box)
            free[y:y + h, x:x + w] = False
        assert int(free.sum()) > 0
        Ns = network_config(name).cas.num_samples[i]
        raw = got[f"net_output_level{i}"][0].cpu().double()[free.reshape(-1)]
        assert float(raw[:, :-Ns].abs().max()) == 0.0
        bg = raw[:, -Ns:]                                                       # (n, Ns, 4): the background's samples alone
        alpha = 1.0 - torch.exp(-bg[..., 3])
        T = torch.cat([torch.ones_like(alpha[:, :1]), torch.cumprod(1.0 - alpha + 1e-10, -1)[:, :-1]], -1)
        bg_rgb = ((alpha * T)[..., None] * bg[..., :3]).sum(-2)
        rgb = got[f"rgb_level{i}"][0].cpu().double()[free.reshape(-1)]
        assert float((rgb - bg_rgb).abs().max()) <= 1e-5 * float(bg_rgb.abs().max()), (name, i)

