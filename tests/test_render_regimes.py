"""The render kernel alone (enerf_render_rays) against the oracle in float64, over every instantiation its launcher can pick, with
the sample range widened until samples leave the source images and the volume; the persistent tile deal and the device-side ray
selection bit for bit.

Which kernel launch_render_rays (csrc/render.hip) picks, and the test here that launches it (a launcher change that moves a
row shows which of these lost its kernel):

    F (level)   n_samples  render_precision  kernel                                   launched by
    11 (1)      1, 2       0 / 1             k_render_rays<3,S,12,3,false,true>       test_render_matches_float64[1-*] (Ns 1, 2), row "l1_lean"
    11 (1)      1, 2       2                 k_render_rays<3,S,12,3,false,true,3>     test_render_precision_variants (B = 2 at S = 3), row "l1_bf16x3"
    11 (1)      1, 2       3                 k_render_rays<3,S,12,3,false,true,6>     test_render_precision_variants (B = 2 at S = 3), row "l1_bf16x6"
    11 (1)      3 .. 8     any               k_render_rays<3,S,4,2,false,false>       test_render_matches_float64[1-*] (Ns 3..8), row "l1_wide"
    35 (0)      1 .. 8     any               k_render_rays<9,S,8,2,false,lean>        test_render_matches_float64[0-*], row "l0"

(Template arguments: R, S, waves per block, waves per SIMD, sample prefetch, lean register set, bf16 split.  lean is ENERF_R9_LEAN,
on by default.  A build with ENERF_RENDER_PREFETCH set would turn the "l1_wide" row at n_samples > 1 into <3,S,4,2,true,false>;
it is off by default and no test builds it.)

Inputs: 32 x 64 source images (enerf_amd.synth.make_batch), the oracle's FeatureNet maps, a random (B, 8, 8, h, w) volume, the
batch's rays with some dropped (N is no multiple of the 16-ray tile).  Both ray forms: 12-float rays whose range columns are
overwritten with [0.2 .. 1 x near, 1 .. 3 x far] per ray (view bounds untouched: samples leave the volume in depth as well as
the images), and 8-float rays with ``maps=`` (the fused build_rays), where all four bounds come from the maps, so the wide range
goes into the near_far map and depth +- std is clipped by it for about half of the pixels.

Reference: oracle.render_rays with every floating input and weight in float64.  Yardstick: the same call in fp32.  Per output
tensor, e = max|x - f64| / max|f64|, and  e_hip <= max(TAU, 3 e_ref).  No ray is masked: where an ill-conditioned ray moves
torch's own fp32 evaluation (up to 1.2e-4 at level 0 with B = 2), the 3 e_ref term is what admits the kernel's.

TAU: five times the worst e_ref over this file's case list, rounded up to one digit (the rule of MLP_TAU in
test_kernel_regimes.py); e_ref is the fp32 oracle's own error and does not involve the kernel.  Measured over the 12 x 8 x 2
float64 cases and the tiny ray lists: worst e_ref 8.9e-7 (F = 11, S = 2, Ns = 1, rgb), so TAU = 5e-6; worst e_hip 1.0e-6 on the
emulator (F = 11, S = 4, Ns = 3, rgb).  (With these seeds no ray is as ill-conditioned as the worst ones found by hand: the
3 e_ref term never decides a case here.)  The precision cases, worst over the six on the emulator: fp32 9.0e-7, bf16x6 8.5e-7,
bf16x3 5.5e-6.
Run time: about 140 s for the CPU entries (the emulated n_samples list is thinned to 1, 2, 3, 5, 8).
"""
import functools
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

from enerf_amd.config import EnerfConfig
from enerf_amd.synth import make_batch
from oracle import enerf_oracle as O

TAU = 5e-6
H, W = 32, 64
CAS = EnerfConfig().cas                           # the default cascade: level 0 F = 35, depth_inv; level 1 F = 11
ROWS = {            # kernel row -> (level, n_samples, render_precision)
    "l1_lean": (1, 2, 0), "l1_bf16x3": (1, 2, 2), "l1_bf16x6": (1, 2, 3), "l1_wide": (1, 5, 0), "l0": (0, 8, 0)}
ROW_WAVES = {"l1_lean": (12, 1), "l1_bf16x3": (12, 1), "l1_bf16x6": (12, 1), "l1_wide": (4, 2), "l0": (8, 1)}   # waves per block, blocks per CU
KEYS = ("rgb", "depth", "weights")
WORST = {"e_ref": 0.0, "e_hip": 0.0}


def _emu():
    from emu_lib import emu_lib
    return emu_lib(), torch.device("cpu")


def _gpu():
    from enerf_amd.lib import get_lib
    return get_lib(), torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _net(vda, gpu):
    """A seeded network (non-trivial biases) on the emulated or the real library, and its state dict for the oracle."""
    from __graft_entry__ import _seeded_network
    lib, dev = _gpu() if gpu else _emu()
    net = _seeded_network(EnerfConfig(viewdir_agg=vda), dev, lib=lib)
    return net, {k: v.detach().cpu() for k, v in net.state_dict().items()}


@functools.lru_cache(maxsize=None)
def _feature_weights():
    from __graft_entry__ import _seeded_network
    return {k: v.detach() for k, v in _seeded_network(EnerfConfig(), torch.device("cpu")).state_dict().items()}


@functools.lru_cache(maxsize=None)
def _scene(S, B):
    """Batch (CPU tensors) and the oracle's FeatureNet maps of its source images."""
    batch = {k: torch.from_numpy(v) for k, v in make_batch(H, W, S, EnerfConfig(), seed=40 + S, B=B, textured=True).items()}
    with torch.no_grad():
        feats = O.forward_feat(_feature_weights(), batch["src_inps"])
    return batch, feats


def _inputs(level, S, B, N, seed):
    """rays8 (B,N,8), maps (depth, std, near_far) at the level's volume size, rays12 with the wide per-ray range, the 12-float
    rays the maps give (what the fused build_rays must reproduce), and the volume (B,8,8,h,w).  All CPU fp32."""
    batch, _ = _scene(S, B)
    g = torch.Generator().manual_seed(seed)
    hv, wv = int(H * CAS.volume_scale[level]), int(W * CAS.volume_scale[level])
    inv = CAS.depth_inv[level]
    vol = torch.randn(B, 8, 8, hv, wv, generator=g)
    rnd = lambda *s: torch.rand(*s, generator=g)
    near, far = batch["near_far"][:, 0], batch["near_far"][:, 1]

    def wide_range(shape):
        e = (1,) * (len(shape) - 1)
        lo, hi = 0.2 + 0.8 * rnd(*shape), 1.0 + 2.0 * rnd(*shape)
        zn, zf = lo * near.view(B, *e), hi * far.view(B, *e)
        return (1.0 / zn, 1.0 / zf) if inv else (zn, zf)          # level 0 places its samples in inverse depth

    rn_m, rf_m = wide_range((B, hv, wv))
    nf = torch.stack([rn_m, rf_m], 1)
    depth = rn_m + (rf_m - rn_m) * rnd(B, hv, wv)
    std = (rf_m - rn_m).abs() * rnd(B, hv, wv) * 0.6              # depth +- std crosses the near_far clip at about half of the pixels
    full = batch[f"rays_{level}"]
    n_full = full.shape[1]
    idx = torch.randperm(n_full, generator=g)[:N] if N <= n_full else torch.randint(0, n_full, (N,), generator=g)
    rays8 = full[:, idx].contiguous()
    with torch.no_grad():
        rays12_maps = O.build_rays(EnerfConfig(), depth, std, {f"rays_{level}": rays8}, nf, level).contiguous()
    rays12 = rays12_maps.clone()
    rays12[..., 8], rays12[..., 9] = wide_range((B, N))
    return dict(rays8=rays8, maps=(depth.contiguous(), std.contiguous(), nf.contiguous()), rays12=rays12, rays12_maps=rays12_maps, vol=vol)


def _prep(lib, dev, net, level, S, B, vol):
    """Device-side operands of the render entry that do not depend on the rays."""
    batch, feats = _scene(S, B)
    im = feats[f"level_{CAS.render_im_feat_level[level]}"].to(dev)
    Hr, Wr = int(H * CAS.render_scale[level]), int(W * CAS.render_scale[level])
    _, _, Cf, Hf, Wf = im.shape
    tex = lib.pack_img_feat_rgb(im.reshape(B * S, Cf, Hf, Wf).contiguous(), batch["src_inps"].to(dev).reshape(B * S, 3, H, W).contiguous(), Hr, Wr)
    tex = tex.view(B, S, Hr, Wr, tex.shape[-1])
    _, _, D, h, w = vol.shape
    vol_cl = lib.channels_last(vol.to(dev).contiguous(), B, 8, D * h * w).view(B, D, h, w, 8)
    cams = [batch[k].to(dev).contiguous() for k in ("src_exts", "src_ixts", "tar_ext")]
    return dict(lib=lib, dev=dev, tex=tex, vol=vol_cl, cams=cams, packed=net._packed_weights(f"nerf_{level}"), level=level)


def _render(p, rays, ns, wb=False, maps=None, precision=0, **kw):
    from enerf_amd.lib import Options
    level = p["level"]
    if maps is not None:
        maps = tuple(m.to(p["dev"]) for m in maps)
    return p["lib"].render_rays(rays.to(p["dev"]).contiguous(), p["tex"], p["vol"], *p["cams"], p["packed"], n_samples=ns,
                                depth_inv=CAS.depth_inv[level], F=CAS.nerf_model_feat_ch[level] + 3, render_scale=CAS.render_scale[level],
                                white_bkgd=wb, maps=maps, options=Options(render_precision=precision) if precision else None, **kw)


def _oracle(sd, level, S, B, rays12, vol, ns, vda, wb, dtype):
    batch, feats = _scene(S, B)
    cast = lambda t: t.to(dtype) if t.is_floating_point() else t
    cfg = EnerfConfig(viewdir_agg=vda, white_bkgd=wb).with_cas(num_samples=(ns, ns))
    with torch.no_grad():
        return O.render_rays(cfg, {k: cast(v) for k, v in sd.items()}, cast(rays12), level, {k: cast(v) for k, v in batch.items()},
                             cast(feats[f"level_{CAS.render_im_feat_level[level]}"]), cast(vol))


def _errors(hip, r64, r32):
    """{tensor: (e_hip, e_ref)}: max|x - f64| / max|f64| for the kernel and for torch fp32."""
    out = {}
    for k, h in zip(KEYS, hip):
        ref = r64[k]
        assert h.shape == ref.shape, (k, h.shape, ref.shape)
        scale = float(ref.abs().max())
        out[k] = (float((h.cpu().double() - ref).abs().max()) / scale, float((r32[k].double() - ref).abs().max()) / scale)
    return out


def _check_float64(tag, hip, r64, r32):
    for k, (e_hip, e_ref) in _errors(hip, r64, r32).items():
        WORST["e_ref"], WORST["e_hip"] = max(WORST["e_ref"], e_ref), max(WORST["e_hip"], e_hip)
        print(f"[render] {tag} {k}: e_hip {e_hip:.2e} e_ref {e_ref:.2e}")
        assert e_hip <= max(TAU, 3.0 * e_ref), f"{tag}: {k} e_hip {e_hip:.3e} > max({TAU:.0e}, 3 x e_ref {e_ref:.3e})"


def _float64_case(gpu, level, S, vda, ns_list):
    """One (level, S, viewdir_agg): every n_samples, both ray forms, white_bkgd both ways (the two forms take opposite values,
    swapped from one n_samples to the next); B = 2 (two rigs) at S = 3, which reaches every kernel row."""
    lib, dev = _gpu() if gpu else _emu()
    net, sd = _net(vda, gpu)
    B = 2 if S == 3 else 1
    N = (117 if level == 0 else 213) if B == 1 else (101 if level == 0 else 107)         # no multiple of 16, nor is B * N
    for ns in ns_list:
        x = _inputs(level, S, B, N, seed=1000 * level + 100 * S + 10 * ns + int(vda))
        p = _prep(lib, dev, net, level, S, B, x["vol"])
        for form, wb in (("rays12", bool(ns & 1)), ("maps", not ns & 1)):
            r12 = x["rays12"] if form == "rays12" else x["rays12_maps"]
            hip = _render(p, r12, ns, wb) if form == "rays12" else _render(p, x["rays8"], ns, wb, maps=x["maps"])
            r64 = _oracle(sd, level, S, B, r12, x["vol"], ns, vda, wb, torch.float64)
            r32 = _oracle(sd, level, S, B, r12, x["vol"], ns, vda, wb, torch.float32)
            _check_float64(f"F={CAS.nerf_model_feat_ch[level] + 3} S={S} B={B} Ns={ns} vda={int(vda)} wb={int(wb)} {form}", hip, r64, r32)
    print(f"[render] worst so far: e_ref {WORST['e_ref']:.2e} e_hip {WORST['e_hip']:.2e}")


def _tiny_n_case(gpu, row):
    """N = 1, 15, 17: one lane, one ragged tile, one tile and one ray."""
    level, ns, _ = ROWS[row]
    lib, dev = _gpu() if gpu else _emu()
    net, sd = _net(True, gpu)
    for N in (1, 15, 17):
        x = _inputs(level, 3, 1, N, seed=7000 + 10 * level + N)
        p = _prep(lib, dev, net, level, 3, 1, x["vol"])
        hip = _render(p, x["rays12"], ns)
        r64 = _oracle(sd, level, 3, 1, x["rays12"], x["vol"], ns, True, False, torch.float64)
        r32 = _oracle(sd, level, 3, 1, x["rays12"], x["vol"], ns, True, False, torch.float32)
        _check_float64(f"{row} N={N}", hip, r64, r32)


def _precision_case(gpu, S, ns, B):
    """render_precision 2 (bf16x3) and 3 (bf16x6) under the bar of test_emu_pipeline.py::
    test_render_precision_variants_match_reference_goldens, on the same wide-range rays as the float64 cases (samples leave the
    images and the volume): every tensor within 2e-5 of the reference (float64 here) in all three modes, bf16x6 as close as
    the exact kernel, bf16x3 no closer than it.  B = 2 (two rigs) at S = 3: the camera block and the target centres lie
    behind the bf16 weight image in LDS, and their size depends on B."""
    lib, dev = _gpu() if gpu else _emu()
    net, sd = _net(True, gpu)
    x = _inputs(1, S, B, 213 if B == 1 else 107, seed=8000 + 10 * S + ns)
    p = _prep(lib, dev, net, 1, S, B, x["vol"])
    r64 = _oracle(sd, 1, S, B, x["rays12"], x["vol"], ns, True, False, torch.float64)
    r32 = _oracle(sd, 1, S, B, x["rays12"], x["vol"], ns, True, False, torch.float32)
    err = {}
    for tag, prec in (("fp32", 0), ("bf16x3", 2), ("bf16x6", 3)):
        err[tag] = {k: e[0] for k, e in _errors(_render(p, x["rays12"], ns, precision=prec), r64, r32).items()}
    print(f"[render] precision S={S} Ns={ns} B={B}: {err}")
    for k in KEYS:
        assert max(err[t][k] for t in err) < 2e-5, (S, ns, B, k, err)
        assert err["bf16x6"][k] <= max(3.0 * err["fp32"][k], 2e-6), (S, ns, B, k, err)
    assert err["fp32"]["rgb"] <= err["bf16x3"]["rgb"], (S, ns, B, err)


def _bulk(level, N, seed, B=1):
    x = _inputs(level, 3, B, N, seed)
    return x["rays12"], x["vol"]


def _same(a, b, what):
    for k, u, v in zip(KEYS, a, b):
        assert torch.equal(u, v), (what, k, float((u - v).abs().max()))


def _max_blocks_case(gpu, row):
    """Every 16-ray tile is computed on its own, so which block and pass renders it cannot change a bit: a launch capped at 1, 3
    and 9 blocks against the uncapped one.  1269 rays = 80 tiles: 3 blocks of 12 waves make two full rounds and a partial
    one, 3 blocks of 8 waves three and a partial one, 9 blocks of 4 waves two and a partial one."""
    level, ns, prec = ROWS[row]
    lib, dev = _gpu() if gpu else _emu()
    net, _ = _net(True, gpu)
    B = 2 if level == 0 else 1                                    # (level 0 has 128 rays per image: the list repeats them, with other ranges)
    # (on the emulator the bf16 modes and the 8-sample level-0 kernel are slow: 26 tiles there, which still gives a single block
    # of 12 waves two full rounds and a partial one, and three blocks of 8 waves one and a partial one)
    n = 1269 if gpu or row in ("l1_lean", "l1_wide") else 413
    rays, vol = _bulk(level, n if B == 1 else n // 2 + 1, 9000 + level, B)
    p = _prep(lib, dev, net, level, 3, B, vol)
    ref = _render(p, rays, ns, precision=prec)
    for mb in (1, 3, 9):
        _same(_render(p, rays, ns, precision=prec, max_blocks=mb), ref, (row, "max_blocks", mb))
    return p, rays, ref


def _selection_case(gpu, row):
    """ray_index / ray_count (B = 1): the entry renders rays ray_index[:count] and writes depth, weights and (without
    scatter_rgb) rgb to rows [0, count), bit for bit what a render of the gathered rays gives.  With scatter_rgb, rgb row
    ray_index[r] gets that value instead — except at count <= 1, where rgb is not written at all (the reference's
    ``mask.sum() > 1``).  Every row the entry does not write is left as the caller passed it: the buffers go in filled with a
    sentinel and must still hold it there (a caller that wants zeros outside the selection zeroes rgb itself, as the frame
    driver does)."""
    level, ns, prec = ROWS[row]
    lib, dev = _gpu() if gpu else _emu()
    net, _ = _net(True, gpu)
    N = 331
    rays, vol = _bulk(level, N, 9100 + level)
    p = _prep(lib, dev, net, level, 3, 1, vol)
    g = torch.Generator().manual_seed(5)
    SENT = -7.0
    for count in (0, 1, 17, N - 37):
        perm = torch.randperm(N, generator=g)
        index = perm.to(torch.int32).to(dev)                       # entries past count are valid positions too, and must not be rendered
        cnt = torch.tensor([count], dtype=torch.int32, device=dev)
        sel = perm[:count]
        want = _render(p, rays[:, sel], ns, precision=prec) if count else None
        for scatter in (False, True):
            out = tuple(torch.full(s, SENT, device=dev) for s in ((1, N, 3), (1, N), (1, N, ns)))
            got = _render(p, rays, ns, precision=prec, ray_index=index, ray_count=cnt, scatter_rgb=scatter, out=out)
            assert all(a is b for a, b in zip(got, out))
            rgb, depth, weights = (t.cpu() for t in got)
            assert (depth[:, count:] == SENT).all() and (weights[:, count:] == SENT).all(), (row, count, scatter)
            if count:
                assert torch.equal(depth[:, :count], want[1].cpu()) and torch.equal(weights[:, :count], want[2].cpu()), (row, count, scatter)
            if not scatter:
                assert (rgb[:, count:] == SENT).all(), (row, count)
                if count:
                    assert torch.equal(rgb[:, :count], want[0].cpu()), (row, count)
            elif count <= 1:
                assert (rgb == SENT).all(), (row, count)
            else:
                assert torch.equal(rgb[0, sel], want[0].cpu()[0]), (row, count)
                rest = torch.ones(N, dtype=torch.bool)
                rest[sel] = False
                assert (rgb[0, rest] == SENT).all(), (row, count)


FLOAT64_CASES = [(level, S, vda) for level in (0, 1) for S in (2, 3, 4) for vda in (True, False)]
TINY_ROWS = ["l1_lean", "l1_wide", "l0"]
PRECISION_CASES = [(S, ns, 1) for S in (2, 4) for ns in (1, 2)] + [(3, 1, 2), (3, 2, 2)]


# ---------------------------------------------------------------------------------------------------------------------------------
# emulator
@pytest.mark.parametrize("level,S,vda", FLOAT64_CASES)
def test_render_matches_float64_emulated(level, S, vda):
    _float64_case(False, level, S, vda, (1, 2, 3, 5, 8))          # (thinned for the emulator's speed; the GPU twin runs all eight)


@pytest.mark.parametrize("row", TINY_ROWS)
def test_render_tiny_ray_lists_emulated(row):
    _tiny_n_case(False, row)


@pytest.mark.parametrize("S,ns,B", PRECISION_CASES)
def test_render_precision_variants_emulated(S, ns, B):
    _precision_case(False, S, ns, B)


@pytest.mark.parametrize("row", list(ROWS))
def test_render_tile_deal_is_bit_identical_emulated(row):
    """max_blocks 0 / 1 / 3 / 9, and the library sized for 1 and 3 CUs against 256."""
    from emu_lib import emu_cu_count
    p, rays, ref = _max_blocks_case(False, row)
    level, ns, prec = ROWS[row]
    for cus in (1, 3):
        with emu_cu_count(p["lib"], cus):
            _same(_render(p, rays, ns, precision=prec), ref, (row, "cus", cus))


@pytest.mark.parametrize("row", list(ROWS))
def test_render_ray_selection_emulated(row):
    _selection_case(False, row)


def test_render_rejects_unusable_out_buffers():
    """out= is written through raw pointers: a wrong shape, type or layout must raise before the launch."""
    from enerf_amd.lib import EnerfError
    lib, dev = _emu()
    net, _ = _net(True, False)
    rays, vol = _bulk(1, 17, 9300)
    p = _prep(lib, dev, net, 1, 3, 1, vol)
    good = lambda: [torch.zeros(1, 17, 3), torch.zeros(1, 17), torch.zeros(1, 17, 2)]
    _render(p, rays, 2, out=tuple(good()))
    for i, bad in ((0, torch.zeros(1, 17, 3, dtype=torch.float64)), (1, torch.zeros(1, 34)[:, ::2]), (2, torch.zeros(1, 17, 4)[..., ::2]),
                   (2, torch.zeros(1, 17, 3))):
        out = good()
        out[i] = bad
        with pytest.raises(EnerfError):
            _render(p, rays, 2, out=tuple(out))


# ---------------------------------------------------------------------------------------------------------------------------------
# MI355X
@pytest.mark.gpu
@pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a GPU")
@pytest.mark.parametrize("level,S,vda", FLOAT64_CASES)
def test_render_matches_float64_on_gpu(level, S, vda):
    _float64_case(True, level, S, vda, range(1, 9))


@pytest.mark.gpu
@pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a GPU")
@pytest.mark.parametrize("row", TINY_ROWS)
def test_render_tiny_ray_lists_on_gpu(row):
    _tiny_n_case(True, row)


@pytest.mark.gpu
@pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a GPU")
@pytest.mark.parametrize("S,ns,B", PRECISION_CASES)
def test_render_precision_variants_on_gpu(S, ns, B):
    _precision_case(True, S, ns, B)


@pytest.mark.gpu
@pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a GPU")
@pytest.mark.parametrize("row", list(ROWS))
def test_render_tile_deal_is_bit_identical_on_gpu(row):
    """max_blocks as on the emulator; then one launch with enough rays for two full rounds of the device's resident waves plus
    a ragged third (N from the CU count), against the same rays rendered one block's worth (16 x waves-per-block rays) at a
    time: such a launch is a single block whose every wave renders one tile at most."""
    _max_blocks_case(True, row)
    level, ns, prec = ROWS[row]
    lib, dev = _gpu()
    net, _ = _net(True, True)
    waves, occ = ROW_WAVES[row]
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    resident = cus * occ * waves
    tiles = 2 * resident + resident // 3 + 1
    N = 16 * tiles - 5
    rays, vol = _bulk(level, N, 9200 + level)
    p = _prep(lib, dev, net, level, 3, 1, vol)
    rays = rays.to(dev)
    whole = _render(p, rays, ns, precision=prec)
    step = 16 * waves
    parts = [_render(p, rays[:, i:i + step], ns, precision=prec) for i in range(0, N, step)]
    _same(whole, tuple(torch.cat([q[i] for q in parts], 1) for i in range(3)), (row, "chunks", N, cus))


@pytest.mark.gpu
@pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a GPU")
@pytest.mark.parametrize("row", list(ROWS))
def test_render_ray_selection_on_gpu(row):
    _selection_case(True, row)
