"""Shared by tests/test_ingest_raw.py (CPU lane emulator) and tests/test_ingest_raw_gpu.py (MI355X): the cases of
``enerf_ingest_raw_u8`` and its float64 numpy restatement, written from the specification in include/enerf_hip.h (not from the kernel):

  x = u8 / 255;  keep_raw = dilate(mask != 0)
  undistort: (u,v) samples the raw image at (u',v') = K . distort(K^-1 (u,v)), bilinear, taps outside contribute 0; the mask is kept
      where the weight of its kept taps is >= 0.5
  resize: Hs, Ws half-to-even; s = 1/r; output d averages the pixels j by |[d s,(d+1) s) n [j,j+1) n [0,src)| normalised, separably;
      the mask takes j = min(floor(d s), src-1)
  crop, x[!keep] = 0, 2x - 1

The value bound against it, absolute on the [-1,1] output, is (2 (9 + n) + 1) 2^-24 with n the largest number of undistorted pixels
under one output pixel of the case: 7 float32 roundings for the bilinear sample of correctly rounded values, 2 for the weights, n for
the sum, doubled by 2x - 1 (plus its own rounding).  Every reference here is computed on the CPU."""
import numpy as np
import torch

DCOEF = (-0.25, 0.12, 0.003, -0.002, -0.03)            # a moderate barrel distortion with tangential terms
STRONG = (2.5, 0.0, 0.0, 0.0, 0.0)                     # pincushion strong enough to push the image's rim outside the raw frame


def bound(n):
    return (2 * (9 + n) + 1) * 2.0 ** -24


def geometry(Hraw, Wraw, r):
    return int(round(Hraw * r)), int(round(Wraw * r))   # Python's round: half to even


def intrinsics(Hraw, Wraw, off=(0.0, 0.0), f=0.9):
    """A plausible pinhole matrix for an Hraw x Wraw frame: focal length f * Wraw, principal point at the centre + ``off``."""
    return np.array([[f * Wraw, 0.0, Wraw / 2 + off[0]], [0.0, 1.03 * f * Wraw, Hraw / 2 + off[1]], [0.0, 0.0, 1.0]], np.float32)


def raw_frame(V, Hraw, Wraw, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (V, Hraw, Wraw, 3), generator=g, dtype=torch.uint8)


def blob_mask(V, Hraw, Wraw, seed):
    """A foreground box per view with a hole, a few lone pixels, and view-dependent nonzero values (``!= 0`` is the test)."""
    rng = np.random.default_rng(seed)
    m = np.zeros((V, Hraw, Wraw), np.uint8)
    for v in range(V):
        y0, x0 = rng.integers(0, Hraw // 3), rng.integers(0, Wraw // 3)
        m[v, y0:y0 + Hraw // 2, x0:x0 + Wraw // 2] = rng.integers(1, 256)
        m[v, y0 + Hraw // 8:y0 + Hraw // 8 + 3, x0 + Wraw // 8:x0 + Wraw // 8 + 5] = 0
        m[v, rng.integers(0, Hraw, 4), rng.integers(0, Wraw, 4)] = 255
    return torch.from_numpy(m)


# -- the float64 restatement ---------------------------------------------------------------------------
def _area_matrix(src, dst, s):
    """(dst, src) float64: row d holds the normalised overlaps of [d s, (d+1) s) with the pixels [j, j+1), inside [0, src)."""
    A = np.zeros((dst, src), np.float64)
    for d in range(dst):
        lo, hi = min(d * s, float(src)), min((d + 1) * s, float(src))
        for j in range(int(np.floor(lo)), int(np.ceil(hi))):
            A[d, j] = max(min(hi, j + 1.0) - max(lo, float(j)), 0.0)
        A[d] /= A[d].sum()
    return A


def _dilate(keep, dilate):
    """(Hraw,Wraw) bool: a dilate x dilate box of ones anchored at its centre, pixels outside the image do not count."""
    if not dilate:
        return keep
    r, (H, W) = dilate // 2, keep.shape
    out = np.zeros_like(keep)
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            ys, xs = slice(max(dy, 0), H + min(dy, 0)), slice(max(dx, 0), W + min(dx, 0))
            yd, xd = slice(max(-dy, 0), H + min(-dy, 0)), slice(max(-dx, 0), W + min(-dx, 0))
            out[yd, xd] |= keep[ys, xs]
    return out


def _taps(K, D, Hraw, Wraw):
    """The four bilinear taps of every undistorted pixel: [(y index, x index, weight (0 where the tap is outside))] float64."""
    K, D = np.asarray(K, np.float64), np.asarray(D, np.float64)
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    k1, k2, p1, p2, k3 = D
    v, u = np.meshgrid(np.arange(Hraw, dtype=np.float64), np.arange(Wraw, dtype=np.float64), indexing="ij")
    with np.errstate(all="ignore"):
        a, b = (u - cx) / fx, (v - cy) / fy
        r2 = a * a + b * b
        rad = 1 + r2 * (k1 + r2 * (k2 + r2 * k3))
        a2 = a * rad + 2 * p1 * a * b + p2 * (r2 + 2 * a * a)
        b2 = b * rad + p1 * (r2 + 2 * b * b) + 2 * p2 * a * b
        us, vs = fx * a2 + cx, fy * b2 + cy
        ok = np.isfinite(us) & np.isfinite(vs)
        ok &= (np.where(ok, us, 0) > -1) & (np.where(ok, us, 0) < Wraw) & (np.where(ok, vs, 0) > -1) & (np.where(ok, vs, 0) < Hraw)
    us, vs = np.where(ok, us, -5.0), np.where(ok, vs, -5.0)              # (-5: every tap outside)
    x0, y0 = np.floor(us), np.floor(vs)
    ax, ay = us - x0, vs - y0
    taps = []
    for dy in (0, 1):
        for dx in (0, 1):
            x, y = (x0 + dx).astype(np.int64), (y0 + dy).astype(np.int64)
            inside = (x >= 0) & (x < Wraw) & (y >= 0) & (y < Hraw)
            w = (ax if dx else 1 - ax) * (ay if dy else 1 - ay)
            taps.append((np.clip(y, 0, Hraw - 1), np.clip(x, 0, Wraw - 1), np.where(inside, w, 0.0)))
    return taps


def restate(img, K=None, D=None, mask=None, dilate=0, r=1.0, crop=None):
    """img (V,Hraw,Wraw,3) uint8, K (V,3,3), D (V,5) or None, mask (V,Hraw,Wraw) or None ->
    dict(out (V,3,H,W) float64, keep (V,H,W) bool, tie (V,H,W) bool: the mask's weight sum within 1e-9 of 0.5, n)."""
    img = img.cpu().numpy()
    V, Hraw, Wraw, _ = img.shape
    Hs, Ws = geometry(Hraw, Wraw, r)
    y0, x0, H, W = (0, 0, Hs, Ws) if crop is None else crop
    s = 1.0 / r
    Ay, Ax = _area_matrix(Hraw, Hs, s)[y0:y0 + H], _area_matrix(Wraw, Ws, s)[x0:x0 + W]
    n = int((Ay > 0).sum(1).max() * (Ax > 0).sum(1).max())
    jy = np.minimum(np.floor(np.arange(y0, y0 + H) * s).astype(np.int64), Hraw - 1)
    jx = np.minimum(np.floor(np.arange(x0, x0 + W) * s).astype(np.int64), Wraw - 1)
    out = np.empty((V, 3, H, W), np.float64)
    keep = np.ones((V, H, W), bool)
    tie = np.zeros((V, H, W), bool)
    for v in range(V):
        x = img[v].astype(np.float64) / 255.0                            # (Hraw,Wraw,3)
        kr = None if mask is None else _dilate(mask[v].cpu().numpy() != 0, dilate)
        if D is not None:
            taps = _taps(K[v].cpu().numpy(), D[v].cpu().numpy(), Hraw, Wraw)
            x = sum(w[..., None] * x[yi, xi] for yi, xi, w in taps)
            if kr is not None:
                wsum = sum(w * kr[yi, xi] for yi, xi, w in taps)
                tie_u = np.abs(wsum - 0.5) < 1e-9
                kr = wsum >= 0.5
                tie[v] = tie_u[jy][:, jx]
        small = np.einsum("dy,yxc,ex->cde", Ay, x, Ax)
        if kr is not None:
            keep[v] = kr[jy][:, jx]
            small = np.where(keep[v][None], small, 0.0)
        out[v] = 2 * small - 1
    return dict(out=out, keep=keep, tie=tie, n=n)


# -- running a case -------------------------------------------------------------------------------------
def run(lib, dev, img, K=None, D=None, mask=None, dilate=0, r=1.0, crop=None, want_mask=False):
    to = lambda t: None if t is None else t.to(dev)
    V, Hraw, Wraw, _ = img.shape
    Hs, Ws = geometry(Hraw, Wraw, r)
    H, W = (Hs, Ws) if crop is None else crop[2:]
    mo = torch.full((V, H, W), 7, dtype=torch.uint8, device=dev) if want_mask else None
    out = lib.ingest_raw_u8(to(img), to(K), to(D), to(mask), dilate, r, crop, mask_out=mo)
    return out.cpu(), (None if mo is None else mo.cpu())


def check(lib, dev, name, img, K=None, D=None, mask=None, dilate=0, r=1.0, crop=None):
    """Run a case, compare with the restatement under the derived bound, print worst / bound; returns (out, ref, worst / bound)."""
    out, mo = run(lib, dev, img, K, D, mask, dilate, r, crop, want_mask=mask is not None)
    ref = restate(img, K, D, mask, dilate, r, crop)
    assert out.dtype == torch.float32 and tuple(out.shape) == ref["out"].shape
    ok = ~ref["tie"]
    assert ref["tie"].mean() <= 1e-3, f"{name}: {ref['tie'].sum()} mask pixels tie at 0.5"
    err = np.abs(out.numpy().astype(np.float64) - ref["out"])
    worst = float(err[np.broadcast_to(ok[:, None], err.shape)].max())
    b = bound(ref["n"])
    print(f"{name}: n = {ref['n']}  worst |err| {worst:.3e}  bound {b:.3e}  worst / bound {worst / b:.3f}")
    assert worst <= b, f"{name}: worst |err| {worst:.3e} > bound {b:.3e}"
    if mask is not None:
        got_keep = mo.numpy() != 0
        assert set(np.unique(mo.numpy()).tolist()) <= {0, 1}
        assert np.array_equal(got_keep[ok], ref["keep"][ok]), f"{name}: mask_out differs from the restatement"
        gone = ~ref["keep"] & ok
        assert bool((out.numpy()[np.broadcast_to(gone[:, None], err.shape)] == -1.0).all()), f"{name}: a masked-out pixel is not -1"
    return out, ref, worst / b


def per_view_cameras(V, Hraw, Wraw):
    K = np.stack([intrinsics(Hraw, Wraw, off=(3.5 * v - 2.25, 1.75 - 2.5 * v), f=0.8 + 0.07 * v) for v in range(V)])
    D = np.stack([np.asarray(DCOEF, np.float32) * (1.0 + 0.4 * v) * (-1) ** v for v in range(V)])
    return torch.from_numpy(K), torch.from_numpy(D.astype(np.float32))


def cams(V, Hraw, Wraw, coef=DCOEF, off=(0.0, 0.0)):
    K = torch.from_numpy(np.stack([intrinsics(Hraw, Wraw, off)] * V))
    D = None if coef is None else torch.tensor([coef] * V, dtype=torch.float32)
    return K, D


# (name, Hraw, Wraw, r): the area-only sizes of the specification
AREA_CASES = (("half_40x56", 40, 56, 0.5), ("half_odd_41x55", 41, 55, 0.5), ("three_quarters_48x64", 48, 64, 0.75),
              ("three_quarters_37x53", 37, 53, 0.75), ("quarter_40x56", 40, 56, 0.25))


# -- the raw= wiring of the caches and the player (shared by the emulator and the GPU file) -------------------------------------
def wired_rig(lib, dev, ixts, Hraw, Wraw, r, seed=0):
    """A RawIngest whose adjusted intrinsics are (close to) ``ixts`` (V,3,3) of the output size: raw K = ixts with rows 0,1 / r, a
    per-view distortion."""
    from enerf_amd.raw_ingest import RawIngest
    V = ixts.shape[0]
    K = ixts.clone().double()
    K[:, :2] /= r
    D = torch.tensor([[c * (1.0 + 0.1 * v) for c in DCOEF] for v in range(V)], dtype=torch.float32)
    return RawIngest(K.float().to(dev), D.to(dev), Hraw, Wraw, input_ratio=r, lib=lib)


def raw_time_frames(V, Hraw, Wraw, seeds):
    return [(raw_frame(V, Hraw, Wraw, seed=50 + s), blob_mask(V, Hraw, Wraw, seed=60 + s)) for s in seeds]


def _same_buffers(x, y):
    assert len(x.buffers) == len(y.buffers)
    for p, q in zip(x.buffers, y.buffers):
        assert (p is None) == (q is None) and (p is None or torch.equal(p, q))


def source_cache_case(lib, dev, net, cfg, H=32, W=64, V=5, dilate=5):
    """cache_sources(raw_u8, ..., raw=rig) holds the buffers of cache_sources(rig(raw_u8, masks, dilate), ...); rebuild is in place."""
    from sequence_cases import time_frames
    _, exts, ixts, _ = time_frames(cfg, H, W, V, seeds=(3,))
    exts = exts.to(dev)
    rig = wired_rig(lib, dev, ixts, 2 * H, 2 * W, 0.5)
    assert (rig.H, rig.W) == (H, W)
    (a, ma), (b, mb) = [(u.to(dev), m.to(dev)) for u, m in raw_time_frames(V, 2 * H, 2 * W, (1, 2))]
    fa, fb = rig(a, ma, dilate).clone(), rig(b, mb, dilate).clone()
    assert bool((fa == -1).all(dim=1).any()) and not torch.equal(fa, fb)
    cache = net.cache_sources(a, exts, rig.ixts, ma, dilate=dilate, raw=rig)
    assert (cache.H, cache.W) == (H, W)
    _same_buffers(cache, net.cache_sources(fa, exts, rig.ixts))
    ptrs = [None if t is None else t.data_ptr() for t in cache.buffers]
    st = cache.struct
    assert cache.rebuild(b, masks=mb, dilate=dilate) is cache
    assert ptrs == [None if t is None else t.data_ptr() for t in cache.buffers] and cache.struct is st
    _same_buffers(cache, net.cache_sources(fb, exts, rig.ixts))
    cache.rebuild(fa)                                                    # a float image of the rig's size is taken as it is
    _same_buffers(cache, net.cache_sources(fa, exts, rig.ixts))
    import pytest
    with pytest.raises(ValueError, match=rf"uint8 \({V},{2 * H},{2 * W},3\)"):
        cache.rebuild(a[:, :H, :W].contiguous())                         # a frame of the OUTPUT size is not a raw frame


def composite_cache_case(lib, dev, name="b", rebuild=True):
    """CompositeSourceCache with raw image and raw background: raw 86 x 128 at 0.75 is 64.5 -> 64 (half to even) x 96.
    ``rebuild=False`` (the emulator, where a build of two FeatureNets takes ten seconds) stops after the first comparison."""
    import composite_cache_cases as CC
    r = CC.rig(lib, dev, name)
    V, H, W = CC.V, CC.H, CC.W
    rig = wired_rig(lib, dev, r.views[3].cpu(), 86, 128, 0.75)
    assert (rig.H, rig.W) == (H, W)
    (a, _), (bg, _), (b, _) = [(u.to(dev), m) for u, m in raw_time_frames(V, 86, 128, (5, 6, 7))]
    got = r.net.cache_sources(a, bg, r.views[2], rig.ixts, raw=rig)
    fa, fbg = rig(a).clone(), rig(bg).clone()
    want = r.net.cache_sources(fa, fbg, r.views[2], rig.ixts)
    for k, t in want.named_buffers().items():
        assert torch.equal(got.named_buffers()[k], t), k
    if not rebuild:
        return
    ptrs = {k: t.data_ptr() for k, t in got.named_buffers().items()}
    got.rebuild(b)                                                       # the next raw frame over the kept background
    assert ptrs == {k: t.data_ptr() for k, t in got.named_buffers().items()}
    want = r.net.cache_sources(rig(b).clone(), fbg, r.views[2], rig.ixts)
    for k, t in want.named_buffers().items():
        assert torch.equal(got.named_buffers()[k], t), k


def player_scene(lib, dev, net, cfg, H, W, V, seeds, dilate=5):
    """(player kwargs, raw frames, tar, references of every (time frame, camera) computed beforehand from the float images)."""
    from sequence_cases import CAMERAS, by_hand, time_frames
    _, exts, ixts, tar = time_frames(cfg, H, W, V, seeds=(3,))
    exts, tar = exts.to(dev), {k: v.to(dev) for k, v in tar.items()}
    rig = wired_rig(lib, dev, ixts, 2 * H, 2 * W, 0.5)
    frames = raw_time_frames(V, 2 * H, 2 * W, seeds)
    refs = {}
    for t, (u8, mask) in enumerate(frames):
        views = rig(u8.to(dev), mask.to(dev), dilate).clone()
        for c, idx in enumerate(CAMERAS):
            refs[(t, c)] = {k: v.clone() for k, v in net(by_hand(views, exts, rig.ixts, tar, idx)).items()}
    return rig, exts, frames, tar, refs
