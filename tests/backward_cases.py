"""Helper of tests/test_backward_regimes.py: the case generators of the four backward stage families (cost-volume warp + variance,
depth regression, compositing, render-side gather), their torch twins (tests/torch_twins.py) under autograd in a chosen dtype,
and the comparison every check shares.

The float64 run of a twin is the reference; its float32 run is the yardstick: per case and tensor,
``d32`` = the maximum over ``SEEDS`` input seeds of max|twin32 - twin64| / scale, and a kernel passes when
max|hip - twin64| / scale <= FACTOR * d32 + FLOOR.  FACTOR is what tests/test_kernel_regimes.py grants over torch fp32's own
distance; FLOOR (16 roundings) keeps an exactly-zero yardstick (D = 1, exact-integer coordinates) from failing a one-ulp difference.
``scale`` is max|twin64|, or, where that is below 2^-24 times the product of the tensor's factors' maxima (a reference that is
analytically ~0: the softmax gradient of a one-hot distribution), that product.

Rounding-decided points: the derivative of a bilinear sample in its coordinate jumps at texel edges, so where a float64 sampling
coordinate lies within NEAR * max(1, |coord|) of an integer (or the projection's depth that close to its 1e-6 clamp) a float32
evaluation may take the other cell.  Those voxels / points get a zero upstream gradient on both sides (as _check_mlp_case masks
its ReLU gates); at most max(2, 1e-3 * count) may be masked on the draw the kernels are compared on, which ``capped`` asserts (the
generators are fixed-seed).  A trilinear coordinate that is the same exact integer in float32 and float64 (a ray's pixel on the image
border) is decided by nothing and stays.
"""
import itertools
import types

import torch
import torch.nn.functional as F

import torch_twins as T
from enerf_amd.config import EnerfConfig
from enerf_amd.synth import make_batch

EPS32 = 2.0 ** -24
FACTOR = 4.0
FLOOR = 16 * EPS32
NEAR = 64 * EPS32
SEEDS = 5


# ---- the shared comparison ------------------------------------------------------------------------------------------------------
def scales(ref64, natural):
    out = {}
    for k, r in ref64.items():
        m = float(r.abs().max()) if r.numel() else 0.0
        out[k] = m if m >= EPS32 * natural[k] else natural[k]
    return out


def distance(a, ref64, scale):
    return float((a.double() - ref64).abs().max()) / scale if ref64.numel() else 0.0


def capped(masked, count, what):
    assert masked <= max(2, 1e-3 * count), (what, masked, count)


_YARD = {}


def yardstick(case, dev):
    """(inputs of the first seed, their float64 results, the scales, d32 per tensor) of a case on ``dev``; computed once per
    device and shared by the tests (nothing in it is written to afterwards)."""
    key = (case.key, dev.type)
    if key not in _YARD:
        d32, first = {}, None
        for i in range(SEEDS):
            inp = case.inputs(case.seed0 + 1000 * i, dev)
            r64 = case.twin(inp, torch.float64)
            r32 = case.twin(inp, torch.float32)
            sc = scales(r64, case.natural(inp))
            for k, r in r64.items():
                d32[k] = max(d32.get(k, 0.0), distance(r32[k], r, sc[k]))
            if i == 0:              # the seed the kernels are compared on: not too much of it may be masked
                capped(inp.get("masked", 0), inp["count"], case.label)
                first = (inp, r64, sc)
        _YARD[key] = first + (d32,)
    return _YARD[key]


def bounds(d32):
    return {k: FACTOR * v + FLOOR for k, v in d32.items()}


def compare(case, hip, dev, note=""):
    """Print the case's line (hip and d32 per tensor), then assert every tensor's bound; returns the worst hip / bound."""
    inp, r64, sc, d32 = yardstick(case, dev)
    bd = bounds(d32)
    errs = {k: distance(hip[k], r64[k], sc[k]) for k in r64}
    worst = max(errs[k] / bd[k] for k in r64)
    parts = "; ".join(f"{k} hip {errs[k]:.1e} d32 {d32[k]:.1e}" for k in r64)
    print(f"[{case.family}] {case.label}{note}: masked={inp.get('masked', 0)}/{inp.get('count', 0)}; {parts}; worst hip/bound {worst:.2f}")
    for k in r64:
        assert hip[k].shape == r64[k].shape, (case.label, k)
        assert errs[k] <= bd[k], f"{case.family} {case.label}: {k} rel err {errs[k]:.3e} > {bd[k]:.3e} (d32 {d32[k]:.3e})"
    return worst


def moved(case, dev, ref_defect, keys=None):
    """Sensitivity: the largest (distance of a defective float64 reference from the true one) / bound over the tensors."""
    _, r64, sc, d32 = yardstick(case, dev)
    bd = bounds(d32)
    return max(distance(ref_defect[k], r64[k], sc[k]) / bd[k] for k in (keys or r64))


def leaf(t, dtype=torch.float32):
    """A fresh differentiable copy (``.to`` of the same dtype would hand back the shared input itself)."""
    return t.detach().to(dtype).clone().requires_grad_(True)


def near_integer(c64, lo, hi, c32=None):
    """Where a float64 coordinate is within rounding of an integer inside [lo, hi] (outside, no tap depends on it)."""
    tol = NEAR * c64.abs().clamp_min(1.0)
    hit = ((c64 - c64.round()).abs() <= tol) & (c64 >= lo - tol) & (c64 <= hi + tol)
    if c32 is not None:
        hit &= ~((c32.double() == c64) & (c64 == c64.round()))
    return hit


# ---- 1. cost-volume warp + variance ---------------------------------------------------------------------------------------------
def warp_coords(proj, dv, dtype=torch.float64):
    """p = R [x, y, 1] + T / d and (u, v) = p.xy / max(p.z, 1e-6) of every (b, s, d, y, x) (utils.py:57-95), in ``dtype``."""
    B, D, h, w = dv.shape
    P, d = proj.to(dtype), dv.to(dtype)
    ys, xs = torch.meshgrid(torch.arange(h, dtype=dtype, device=dv.device), torch.arange(w, dtype=dtype, device=dv.device), indexing="ij")
    e = lambda r, c: P[:, :, r, c, None, None, None]
    row = lambda r: e(r, 0) * xs + e(r, 1) * ys + e(r, 2) + e(r, 3) / d[:, None]
    px, py, pz = row(0), row(1), row(2)
    z = pz.clamp_min(1e-6)
    return px, py, pz, px / z, py / z


def _cells(u, v):
    fin = (u.abs() < 1e8) & (v.abs() < 1e8)                      # (NaN compares false)
    x0 = torch.where(fin, u, torch.full_like(u, -10.0)).floor().long()
    y0 = torch.where(fin, v, torch.full_like(v, -10.0)).floor().long()
    return x0, y0


def warp_regime(u, v, Hs, Ws, C):
    """The kernel's regimes restated from the float64 coordinates (B,S,D,h,w), per (voxel, view) in the kernel's voxel order:
    m0 / m1 (S, nvox) — the right neighbour is in the same wave, its (y0, x0) / (y1, x0) texel is my (y0, x1) / (y1, x1) and both
    taps are valid: its left contributions ride on my right atomics — and ``outside``: all four taps outside the image."""
    B, S = u.shape[:2]
    per_b = u[0, 0].numel()
    nvox = B * per_b
    x0, y0 = _cells(u.transpose(0, 1).reshape(S, nvox), v.transpose(0, 1).reshape(S, nvox))
    idx = torch.arange(nvox, device=u.device)
    nvw = 64 // (C // 4)                                           # voxels per wave
    has_r = (idx % nvw < nvw - 1) & (idx < nvox - 1) & (idx // per_b == (idx + 1).clamp_max(nvox - 1) // per_b)
    xr, yr = torch.roll(x0, -1, 1), torch.roll(y0, -1, 1)
    vx = lambda x: (x >= 0) & (x < Ws)
    vy = lambda y: (y >= 0) & (y < Hs)
    same = has_r & (xr == x0 + 1) & (yr == y0) & vx(xr)
    m0, m1 = same & vy(y0), same & vy(y0 + 1)
    outside = ~((vx(x0) | vx(x0 + 1)) & (vy(y0) | vy(y0 + 1)))
    return m0, m1, outside


def warp_taps_volume(feats, proj, dv, keep0=None, keep1=None):
    """The twin's cost volume restated with explicit taps (float64): warped = sum_tap w_tap feats[tap].  keep0 / keep1
    (B,S,D,h,w) bool: where False the (y0, x0) / (y1, x0) tap reads a detached copy — the same value, no gradient into the
    feature maps: the defect of a merged contribution that never arrives."""
    B, S, C, Hs, Ws = feats.shape
    _, D, h, w = dv.shape
    _, _, _, u, v = warp_coords(proj, dv, feats.dtype)
    fin = (u.abs() < 1e8) & (v.abs() < 1e8)
    u, v = torch.where(fin, u, torch.full_like(u, -10.0)), torch.where(fin, v, torch.full_like(v, -10.0))
    x0, y0 = u.detach().floor(), v.detach().floor()
    flat, flat_d = feats.reshape(B, S, C, Hs * Ws), feats.detach().reshape(B, S, C, Hs * Ws)
    warped = 0.0
    for dy, dx in itertools.product((0, 1), (0, 1)):
        xi, yi = (x0 + dx).long(), (y0 + dy).long()
        ok = (xi >= 0) & (xi < Ws) & (yi >= 0) & (yi < Hs)
        wgt = ((u - x0) if dx else (x0 + 1 - u)) * ((v - y0) if dy else (y0 + 1 - v)) * ok
        at = (yi.clamp(0, Hs - 1) * Ws + xi.clamp(0, Ws - 1)).reshape(B, S, 1, -1).expand(B, S, C, -1)
        val = flat.gather(3, at)
        keep = (keep0, keep1)[dy] if dx == 0 else None
        if keep is not None:
            val = torch.where(keep.reshape(B, S, 1, -1), val, flat_d.gather(3, at))
        warped = warped + val * wgt.reshape(B, S, 1, -1)
    warped = warped.view(B, S, C, D, h, w)
    return (warped ** 2).mean(1) - warped.mean(1) ** 2


def _rigid(B, S, fn):
    return torch.tensor([[fn(b, s) for s in range(S)] for b in range(B)], dtype=torch.float32)


def _unit_step(b, s):            # one texel per voxel step: the right neighbour's left taps are my right taps
    return [[1, 0, 0.37 + 0.2 * s - 0.05 * b, 30.0 * (s + 1)], [0, 1, 0.21 + 0.1 * b, -20.0 * (s + 1)], [0, 0, 1, 0]]


def _exact(b, s):
    sg = 1.0 if s == 0 else -1.0
    return [[1, 0, 0, 1024.0 * sg], [0, 1, 0, -512.0 * sg], [0, 0, 1, 0]]


BEHIND_VIEW, NONFINITE_VIEW = 2, 3


def _oblique(b, s):              # rotation 40 + 57 s degrees, scale 1.7; the volume's centre (6, 4) lands on the map's centre (9.5, 5.5)
    import math                  # at the fourth plane (d = 725) — of the clamped view after its division by p.z = 1 - 650 / 725 there
    a = math.radians(40.0 + 57.0 * s)
    c, sn = 1.7 * math.cos(a), 1.7 * math.sin(a)
    if s == NONFINITE_VIEW:
        p3, p7, p11, k = 1e12, -300.0 * (s + 1), 0.0, 1.0
    elif s == BEHIND_VIEW:
        p3, p7, p11, k = 60.0, -45.0, -650.0, 1.0 - 650.0 / 725.0
    else:
        p3, p7, p11, k = 400.0 * (s + 1), -300.0 * (s + 1), 0.0, 1.0
    t3 = 0.0 if p3 > 1e6 else p3 / 725.0
    return [[c, -sn, 9.5 * k - (c * 6 - sn * 4) - t3, p3], [sn, c, 5.5 * k - (sn * 6 + c * 4) - p7 / 725.0, p7], [0, 0, 1, p11]]


class WarpCase:
    family = "warp"
    KINDS = {"unit": dict(B=2, S=3, src=(9, 13), vol=(3, 7, 11), proj=_unit_step),
             "unit_s2": dict(B=2, S=2, src=(9, 13), vol=(3, 7, 11), proj=_unit_step),
             "exact": dict(B=1, S=2, src=(7, 11), vol=(3, 7, 11), proj=_exact),
             "oblique": dict(B=1, S=4, src=(12, 20), vol=(5, 9, 13), proj=_oblique)}

    def __init__(self, kind, C):
        k = self.KINDS[kind]
        self.kind, self.C, self.B, self.S, self.src, self.vol = kind, C, k["B"], k["S"], k["src"], k["vol"]
        self.proj = _rigid(self.B, self.S, k["proj"])
        self.key, self.label = ("warp", kind, C), f"{kind} C={C} B={self.B} S={self.S}"
        self.seed0 = 300 + C + 7 * sorted(self.KINDS).index(kind)

    def inputs(self, seed, dev):
        g = torch.Generator().manual_seed(seed)
        B, S, C, (Hs, Ws), (D, h, w) = self.B, self.S, self.C, self.src, self.vol
        feats = torch.randn(B, S, C, Hs, Ws, generator=g)
        if self.kind == "exact":
            dv = torch.tensor([256.0, 512.0, 1024.0]).view(1, D, 1, 1).expand(B, D, h, w).contiguous()
        else:
            dv = torch.linspace(500.0, 800.0, D).view(1, D, 1, 1).expand(B, D, h, w) + 3.0 * torch.randn(B, D, h, w, generator=g)
        gout = torch.randn(B, C, D, h, w, generator=g)
        inp = dict(feats=feats.to(dev), dv=dv.contiguous().to(dev), proj=self.proj.to(dev), count=B * D * h * w, masked=0)
        _, _, pz, u, v = warp_coords(inp["proj"], inp["dv"])
        inp.update(u=u, v=v, pz=pz)
        if self.kind != "exact":            # (exact: the coordinates are the same exact numbers in both precisions — asserted by the check)
            near = ((near_integer(u, -1, Ws) | near_integer(v, -1, Hs)) & (u >= -2) & (u <= Ws + 1) & (v >= -2) & (v <= Hs + 1)) | \
                ((pz - 1e-6).abs() <= NEAR * pz.abs().clamp_min(1.0))
            near = near.any(1)                                                      # (B,D,h,w)
            inp["masked"] = int(near.sum())
            gout = gout.to(dev) * (~near)[:, None]
        inp["gout"] = gout.to(dev)
        return inp

    def twin(self, inp, dtype, gout=None, fn=None):
        """``fn``: T.feature_volume, except in the exact-integer case.  There the twin cannot arbitrate g_dv: it normalises (u, v) to
        [-1, 1] and grid_sample un-normalises them, which moves an exact integer by an ulp in either precision, so each run
        differentiates in whichever cell its rounding picked (twin32 against twin64: 3.1 of max|g_dv|).  The explicit-tap
        restatement samples at (u, v) themselves; it equals the twin to 1e-12, gradients included, wherever rounding decides
        nothing (asserted on the unit-step case) and keeps ATen's convention at an integer (asserted by the check)."""
        fn = fn or (warp_taps_volume if self.kind == "exact" else T.feature_volume)
        feats, dv = leaf(inp["feats"], dtype), leaf(inp["dv"], dtype)
        vol = fn(feats, inp["proj"].to(dtype), dv)
        vol.backward((inp["gout"] if gout is None else gout).to(dtype))
        return {"volume": vol.detach(), "g_feats": feats.grad, "g_dv": dv.grad}

    def natural(self, inp):
        f, g = float(inp["feats"].abs().max()), float(inp["gout"].abs().max())
        t = inp["proj"][..., 3].abs()
        t = float(t[t < 1e6].max())
        return {"volume": f * f, "g_feats": g * f, "g_dv": g * f * f * t / float(inp["dv"].abs().min()) ** 2}

    def hip(self, lib, inp, b=None):
        """Through FeatureVolumeFn; ``b``: that batch element alone, as a B = 1 launch."""
        from enerf_amd.autograd import FeatureVolumeFn
        sl = slice(None) if b is None else slice(b, b + 1)
        feats, dv = leaf(inp["feats"][sl]), leaf(inp["dv"][sl])
        vol = FeatureVolumeFn.apply(lib, feats, inp["proj"][sl].contiguous(), dv)
        vol.backward(inp["gout"][sl])
        return {"volume": vol.detach(), "g_feats": feats.grad, "g_dv": dv.grad}


# ---- 2. depth regression --------------------------------------------------------------------------------------------------------
DEPTH_PLANES = (1, 3, 8, 16, 17, 30, 48, 63, 64, 65, 96)


class DepthCase:
    family = "depth_regression"
    B, h, w = 2, 3, 7                # 42 pixels, 16 per wave: the second wave straddles the batch elements, the third is partial

    def __init__(self, D, inv, kind="random"):
        self.D, self.inv, self.kind = D, inv, kind
        self.key, self.label = ("depth", D, inv, kind), f"D={D} depth_inv={int(inv)} {kind}"
        self.seed0 = 500 + 2 * D + int(inv) + 37 * ("random", "onehot", "clamped").index(kind)

    def inputs(self, seed, dev):
        g = torch.Generator().manual_seed(seed)
        B, D, h, w = self.B, self.D, self.h, self.w
        prob = torch.randn(B, D, h, w, generator=g)
        dv = 500.0 + 300.0 * torch.rand(B, D, h, w, generator=g)
        inp = dict(count=B * h * w)
        if self.kind == "onehot":                     # +200 on one plane: exp(-200) underflows, float32 p is exactly one-hot
            hot = torch.randint(0, D, (B, 1, h, w), generator=g)
            prob.scatter_add_(1, hot, torch.full((B, 1, h, w), 200.0))
            inp["hot"] = hot.to(dev)
        if self.kind == "clamped":                    # ~10 % of the depths on or below the 1e-6 clamp of 1 / max(dv, 1e-6)
            sel = torch.rand(B, D, h, w, generator=g) < 0.1
            low = torch.tensor([0.0, -3.0, 5e-7])[torch.randint(0, 3, (B, D, h, w), generator=g)]
            dv = torch.where(sel, low, dv)
            inp["clamped"] = sel.to(dev)
        inp.update(prob=prob.to(dev), dv=dv.to(dev), g_depth=torch.randn(B, h, w, generator=g).to(dev),
                   g_std=torch.randn(B, h, w, generator=g).to(dev))
        return inp

    def twin(self, inp, dtype, planes=None):
        cas = types.SimpleNamespace(depth_inv=(self.inv,))
        D = self.D if planes is None else planes
        prob, dv = leaf(inp["prob"][:, :D], dtype), leaf(inp["dv"][:, :D], dtype)
        d, s = T.depth_regression(cas, prob, dv, 0)
        (d * inp["g_depth"].to(dtype) + s * inp["g_std"].to(dtype)).sum().backward()
        return {"depth": d.detach(), "std": s.detach(), "g_prob": prob.grad, "g_dv": dv.grad}

    def natural(self, inp):
        d = inp["dv"].clamp_min(1e-6)
        v = float((1.0 / d).max()) if self.inv else float(d.max())
        g = float(inp["g_depth"].abs().max()) + float(inp["g_std"].abs().max())
        live = inp["dv"][inp["dv"] >= 1e-6]                                         # (a clamped depth receives no gradient)
        return {"depth": v, "std": v, "g_prob": g * v, "g_dv": g * float((1.0 / live ** 2).max()) if self.inv else g}

    def hip(self, lib, inp, g_std=None):
        from enerf_amd.autograd import DepthRegressionFn
        prob, dv = leaf(inp["prob"]), leaf(inp["dv"])
        d, s = DepthRegressionFn.apply(lib, prob, dv, self.inv)
        (d * inp["g_depth"] + s * (inp["g_std"] if g_std is None else g_std)).sum().backward()
        return {"depth": d.detach(), "std": s.detach(), "g_prob": prob.grad, "g_dv": dv.grad}


# ---- 3. compositing -------------------------------------------------------------------------------------------------------------
class CompositeCase:
    family = "composite"

    def __init__(self, Ns, n=300):
        self.Ns, self.n, self.white = Ns, n, bool(Ns % 2)
        self.B, self.N = (2, n // 2) if n % 2 == 0 else (1, n)
        self.key, self.label = ("composite", Ns, n), f"Ns={Ns} n={n} white_bkgd={int(self.white)}"
        self.seed0 = 700 + 11 * Ns + n

    def inputs(self, seed, dev):
        g = torch.Generator().manual_seed(seed)
        B, N, Ns = self.B, self.N, self.Ns
        sigma = 40.0 * torch.rand(B, N, Ns, generator=g) ** 3                              # up to 40, most of it moderate
        sigma = torch.where(torch.rand(B, N, Ns, generator=g) < 0.1, torch.zeros(()), sigma)          # sigma == 0 on a tenth
        sat = torch.randint(0, Ns, (B, N, 1), generator=g)                                 # one saturated sample per ray:
        sigma.scatter_(2, sat, 30.0)                                                       # exp(-30) < 2^-25, alpha == 1 in float32
        assert bool(((1.0 - torch.exp(-sigma)) == 1.0).any(-1).all()) and (Ns == 1 or B * N == 1 or bool((sigma == 0).any()))
        raw = torch.cat([torch.rand(B, N, Ns, 3, generator=g), sigma[..., None]], -1)
        z = 400.0 + 500.0 * torch.rand(B, N, Ns, generator=g)
        gr, gd, gw = torch.randn(B, N, 3, generator=g), 1e-2 * torch.randn(B, N, generator=g), torch.randn(B, N, Ns, generator=g)
        return dict(raw=raw.to(dev), z=z.to(dev), g_rgb=gr.to(dev), g_depth=gd.to(dev), g_weights=gw.to(dev), count=B * N)

    def twin(self, inp, dtype, rays=None):
        """``rays``: only the first ``rays`` rays receive an upstream gradient (the sensitivity defect)."""
        raw, z = leaf(inp["raw"], dtype), leaf(inp["z"], dtype)
        gr, gd, gw = (inp[k].to(dtype).clone() for k in ("g_rgb", "g_depth", "g_weights"))
        if rays is not None:
            for t in (gr, gd, gw):
                t.view(self.B * self.N, -1)[rays:] = 0
        out = T.raw2outputs(raw, z, self.white)
        loss = (out["rgb"] * gr).sum() + (out["depth"] * gd).sum() + (out["weights"] * gw).sum()
        g_raw, = torch.autograd.grad(loss, raw, retain_graph=True)
        assert torch.autograd.grad(loss, z, retain_graph=True, allow_unused=True)[0] is None        # utils.py:595: z_vals.detach()
        g_z, = torch.autograd.grad((((out["weights"] * z).sum(-1)) * gd).sum(), z)           # the un-detached derivative (k_composite_bwd's g_z)
        return {"rgb": out["rgb"].detach(), "depth": out["depth"].detach(), "weights": out["weights"].detach(), "g_raw": g_raw, "g_z": g_z}

    def natural(self, inp):
        zm, gd = float(inp["z"].abs().max()), float(inp["g_depth"].abs().max())
        return {"rgb": 1.0, "depth": zm, "weights": 1.0, "g_z": gd,
                "g_raw": float(inp["g_rgb"].abs().max()) + float(inp["g_weights"].abs().max()) + gd * zm}

    def flat(self, inp):
        n, Ns = self.B * self.N, self.Ns
        return (inp["raw"].reshape(n, Ns, 4), inp["z"].reshape(n, Ns), inp["g_rgb"].reshape(n, 3), inp["g_depth"].reshape(n),
                inp["g_weights"].reshape(n, Ns))

    def hip(self, lib, inp):
        """rgb, depth, weights and g_raw through CompositeFn; g_z (which the Function drops) from lib.composite_bwd."""
        from enerf_amd.autograd import CompositeFn
        raw, z = leaf(inp["raw"]), leaf(inp["z"])
        rgb, depth, wts = CompositeFn.apply(lib, raw, z, self.white)
        ((rgb * inp["g_rgb"]).sum() + (depth * inp["g_depth"]).sum() + (wts * inp["g_weights"]).sum()).backward()
        assert z.grad is None
        g_raw2, g_z = lib.composite_bwd(*self.flat(inp))
        assert torch.equal(g_raw2.view_as(raw), raw.grad)
        return {"rgb": rgb.detach(), "depth": depth.detach(), "weights": wts.detach(), "g_raw": raw.grad, "g_z": g_z.view_as(z)}


# ---- 4. render-side gather ------------------------------------------------------------------------------------------------------
GATHER_ANY = ((1, 11), (2, 35), (3, 4), (4, 16), (3, 17), (2, 48), (3, 49), (4, 11))          # (S, F)
GATHER_RASTER = ((20, 44, 2, 11, 2), (12, 40, 4, 35, 4))                                      # (Hr, Wr, Ns, F, S)


class GatherCase:
    family = "gather"

    def __init__(self, S, Fc, raster=None, hints=False):
        self.S, self.F, self.raster, self.hints = S, Fc, raster, hints
        if raster is None:
            self.Hr, self.Wr, self.Ns, self.N, self.vol = 12, 20, 3, 37, (5, 6, 10)
        else:
            self.Hr, self.Wr, self.Ns = raster
            self.N, self.vol = self.Hr * self.Wr, (8, self.Hr // 2, self.Wr // 2)
        self.B = 2
        self.key = ("gather", S, Fc, raster)             # (with and without hints: the same inputs, the same reference)
        self.label = f"S={S} F={Fc} " + ("any order" if raster is None else f"raster {self.Hr}x{self.Wr} Ns={self.Ns}")
        self.seed0, self.cam_seed = 900 + 13 * S + Fc, 12 + S
        self.cas = EnerfConfig().with_cas(render_scale=(1.0, 1.0)).cas

    def inputs(self, seed, dev):
        g = torch.Generator().manual_seed(seed)
        B, S, Fc, Hr, Wr, Ns, N = self.B, self.S, self.F, self.Hr, self.Wr, self.Ns, self.N
        D, h, w = self.vol
        cfg = EnerfConfig().with_cas(render_scale=(1.0, 1.0))
        b = {k: torch.from_numpy(v) for k, v in make_batch(Hr, Wr, S, cfg, seed=self.cam_seed, B=B).items()}
        near, far = float(b["near_far"].min()), float(b["near_far"].max())
        if self.raster is None:            # as _check_hip_backward_stages: random depths, 30 % of the points pushed sideways out of the images
            pick = torch.stack([torch.randperm(Hr * Wr, generator=g)[:N] for _ in range(B)])
            rays = torch.gather(b["rays_1"], 1, pick[..., None].expand(B, N, b["rays_1"].shape[-1]))
            t = near + (far - near) * torch.rand(B, N, Ns, generator=g)
            side = 120.0 * torch.randn(B, N, Ns, 3, generator=g) * (torch.rand(B, N, Ns, 1, generator=g) < 0.3)
            xyz = (rays[:, :, None, :3] + rays[:, :, None, 3:6] * t[..., None] + side).reshape(B, N * Ns, 3)
            dn = torch.rand(B, N * Ns, generator=g) * 1.3 - 0.15
            uv = torch.rand(B, N * Ns, 2, generator=g) * torch.tensor([Wr - 1.0, Hr - 1.0])
        else:                              # as _check_gather_bwd_tiled: row-major full-image rays on a smooth depth map
            rays = b["rays_1"]
            assert rays.shape[1] == N
            yy, xx = torch.meshgrid(torch.linspace(0, 1, Hr), torch.linspace(0, 1, Wr), indexing="ij")
            base = near + (far - near) * (0.3 + 0.4 * torch.sin(3 * xx + 2 * yy).abs()).reshape(1, N, 1)
            t = base + (far - near) * 0.02 * torch.arange(Ns).reshape(1, 1, Ns) + (far - near) * 0.005 * torch.rand(B, N, Ns, generator=g)
            xyz = (rays[:, :, None, :3] + rays[:, :, None, 3:6] * t[..., None]).reshape(B, N * Ns, 3)
            dn = torch.rand(B, N * Ns, generator=g) * 1.2 - 0.1
            uv = rays[:, :, None, 6:8].expand(B, N, Ns, 2).reshape(B, N * Ns, 2)
        P = N * Ns
        tex, vol = torch.randn(B, S, Hr, Wr, Fc, generator=g), torch.randn(B, D, h, w, 8, generator=g)
        gx, gv = torch.randn(B, P, S, Fc + 4, generator=g), torch.randn(B, P, 8, generator=g)
        cam, tcen = T.gather_cameras(b, 1.0)
        to = lambda t_: t_.contiguous().to(dev)
        inp = dict(xyz=to(xyz), dn=to(dn), uv=to(uv), tex=to(tex), vol=to(vol), cam=to(cam), tcen=to(tcen), count=B * P,
                   batch={k: to(b[k]) for k in ("src_exts", "src_ixts", "tar_ext")})
        near_pt = self.rounding_decided(inp)
        inp["masked"] = int(near_pt.sum())
        inp["g_x"], inp["g_vox"] = to(gx) * (~near_pt)[..., None, None], to(gv) * (~near_pt)[..., None]
        return inp

    def rounding_decided(self, inp):
        """(B,P) bool from the float64 sampling coordinates: the pixel coordinates per view, the projection's depth, the trilinear
        coordinates of the volume sample."""
        E, K = inp["batch"]["src_exts"].double(), inp["batch"]["src_ixts"].double()
        M, t = K @ E[:, :, :3, :3], (K @ E[:, :, :3, 3:4])[..., 0]                         # (B,S,3,3), (B,S,3)
        pix = inp["xyz"].double()[:, None] @ M.transpose(-1, -2) + t[:, :, None]           # (B,S,P,3)
        pz = pix[..., 2]
        z = pz.clamp_min(1e-6)
        ix, iy = pix[..., 0] / z, pix[..., 1] / z
        near = near_integer(ix, 0, self.Wr - 1) | near_integer(iy, 0, self.Hr - 1) | ((pz - 1e-6).abs() <= NEAR * pz.abs().clamp_min(1.0))
        near = near.any(1)
        D, h, w = self.vol
        for c, size_in, size in ((inp["uv"][..., 0], self.Wr, w), (inp["uv"][..., 1], self.Hr, h), (inp["dn"], 2, D)):
            un = lambda x: (((x / (size_in - 1)) * 2.0 - 1.0) + 1.0) * 0.5 * (size - 1)     # (vox_geom: normalise, gs_unnorm)
            near |= near_integer(un(c.double()), -1, size, un(c))
        return near

    def twin(self, inp, dtype, g_x=None):
        B, P = inp["dn"].shape
        xyz, dn, tex, vol = (leaf(inp[k], dtype) for k in ("xyz", "dn", "tex", "vol"))
        uv = inp["uv"].to(dtype)
        nd = torch.stack([uv[..., 0] / (self.Wr - 1), uv[..., 1] / (self.Hr - 1), dn], -1)            # network.py:36-38
        gg = nd.reshape(B, 1, 1, P, 3) * 2.0 - 1.0
        vox = F.grid_sample(vol.permute(0, 4, 1, 2, 3), gg, align_corners=True)[:, :, 0, 0].permute(0, 2, 1)
        batch = {k: v.to(dtype) for k, v in inp["batch"].items()}
        x = T.img_feat(self.cas, xyz.reshape(B, P, 1, 3), tex.permute(0, 1, 4, 2, 3), batch, 1)
        ((x * (inp["g_x"] if g_x is None else g_x).to(dtype)).sum() + (vox * inp["g_vox"].to(dtype)).sum()).backward()
        return {"x": x.detach(), "vox": vox.detach(), "g_xyz": xyz.grad, "g_dn": dn.grad, "g_tex": tex.grad, "g_vol": vol.grad}

    def natural(self, inp):
        tx, vl, gx, gv = (float(inp[k].abs().max()) for k in ("tex", "vol", "g_x", "g_vox"))
        D = self.vol[0]
        return {"x": tx, "vox": vl, "g_tex": gx, "g_vol": gv, "g_dn": gv * vl * (D - 1), "g_xyz": gx * tx}

    def hip(self, lib, inp, hints=False):
        from enerf_amd.autograd import GatherFn
        xyz, dn, tex, vol = (leaf(inp[k]) for k in ("xyz", "dn", "tex", "vol"))
        hint = (self.Ns, self.Wr) if hints else (0, 0)
        x, vox = GatherFn.apply(lib, xyz, dn, inp["uv"], tex, vol, inp["cam"], inp["tcen"], *hint)
        ((x * inp["g_x"]).sum() + (vox * inp["g_vox"]).sum()).backward()
        return {"x": x.detach(), "vox": vox.detach(), "g_xyz": xyz.grad, "g_dn": dn.grad, "g_tex": tex.grad, "g_vol": vol.grad}
